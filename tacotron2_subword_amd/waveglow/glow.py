"""Drop-in for the reference's ``glow.WaveGlow`` (glow.py:178-310) and ``glow.WaveGlowLoss`` (glow.py:43-59) on the MI355X:
inference, the values of the training direction, and -- as an opt-in -- training.

The modules below only hold parameters, under the names and shapes the reference's checkpoints use; ``WaveGlow.infer``
folds the weight norm (g * v / ||v||), inverts the 1x1 mixes once in fp32 (glow.py:91), hands everything to the HIP library
(csrc/waveglow.hip) packed into the order its kernels read, and then runs the whole model through ``t2_waveglow_infer``.
So the reference's lines work verbatim::

    waveglow = torch.load(path)['model']      # or WaveGlow(**waveglow_config) + load_state_dict
    waveglow.cuda().eval()
    with torch.no_grad():
        audio = waveglow.infer(mel, sigma=0.666)      # mel [B, 80, T] fp32 on the GPU -> [B, T * 256]

A module that was pickled whole by the reference (its classes live in a top-level ``glow``) loads once
``sys.modules['glow']`` points at this module; its children are then torch's own Conv1d / ConvTranspose1d, weight-normed or
not, which ``infer`` reads just the same.  Always fp32 (``set_precision`` does not reach the vocoder), no CPU path.

The other direction of the flow, audio -> z (glow.py:207-249, what waveglow/train.py:125-127 calls on every batch), is there as
values without a gradient: ``analyze((mel, audio))`` returns the reference's ``(z, log_s_list, log_det_W_list)``,
``WaveGlowLoss(sigma)`` turns such a tuple into the negative log-likelihood per sample, and ``nll(mel, audio, sigma)`` gives
that number (or one per item) straight from sums the kernels form, for a validation or scoring loop::

    with torch.no_grad():
        loss = waveglow.nll(mel, audio, sigma=1.0)                  # == WaveGlowLoss(1.0)(waveglow.analyze((mel, audio)))

``forward`` / ``__call__`` refuse on a module that has not opted in.  ``WaveGlow.trainable()`` opts in: ``model((mel, audio))`` then
is the reference's forward with a backward (t2_waveglow_train_forward / t2_waveglow_backward), so waveglow/train.py:125-137 runs
with one changed line::

    model = WaveGlow(**waveglow_config).cuda().trainable()
    loss = WaveGlowLoss(sigma)(model((mel, audio)));  loss.backward()     # .grad on every parameter, weight-normed or not

Two things differ from ``analyze`` on that path.  The weight norm is folded on the device by torch's own ``_weight_norm`` (whose
autograd carries the folded gradient on to ``weight_g`` / ``weight_v``), so ``z`` may differ from ``analyze``'s, folded on the host,
in the last bits.  And the parameters change every step, so the weights are packed on every call into a buffer of their own: the
``_key()`` cache is not consulted and ``_packed`` / ``_packed_fwd`` are left alone.  ``B * L * logdet(W_k)`` is torch's autograd too.
Gradients with respect to the mel and the audio, fp16 and amp are not built and refused by name."""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import nn

from .. import _lib as L


# what WaveGlow caches outside its pickled state: inference's packed weights, the analysis direction's and their log|det W_k|
_CACHES = ("_packed", "_packed_key", "_packed_fwd", "_packed_fwd_key", "_logdet_fwd")


class WaveGlowLoss(nn.Module):
    """glow.py:43-59: the negative log-likelihood per sample of ``(z, log_s_list, log_det_W_list)``, in torch ops on any such
    tuple (what ``WaveGlow.analyze`` returns, or the reference's own forward).  ``WaveGlow.nll`` gives the same value from sums
    the kernels make, without the log_s tensors."""

    def __init__(self, sigma=1.0):
        super().__init__()
        self.sigma = sigma

    def forward(self, model_output):
        z, log_s_list, log_det_W_list = model_output
        # the terms are added flow by flow, k ascending, as the reference adds them; its += on log_det_W_list[0] is not repeated
        log_s_total, log_det_total = torch.sum(log_s_list[0]), log_det_W_list[0]
        for log_s, log_det in zip(log_s_list[1:], log_det_W_list[1:]):
            log_s_total, log_det_total = log_s_total + torch.sum(log_s), log_det_total + log_det
        gaussian = torch.sum(z * z) / (2 * self.sigma * self.sigma)
        return (gaussian - log_s_total - log_det_total) / z.numel()


class _Conv(nn.Module):
    """Parameters of a Conv1d [cout, cin, k] (ConvTranspose1d: [cin, cout, k]) under torch's default initialisation.  With
    weight_norm they are ``bias``, ``weight_g`` [cout, 1, 1], ``weight_v``, as torch.nn.utils.weight_norm leaves them; without,
    ``weight``, ``bias``."""

    def __init__(self, cin, cout, k, weight_norm=True, bias=True, transposed=False, dilation=1, stride=1):
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.kernel_size, self.dilation, self.stride = (k,), (dilation,), (stride,)
        w = torch.empty((cin, cout, k) if transposed else (cout, cin, k))
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(w.shape[1] * k)
        if not weight_norm:
            self.weight = nn.Parameter(w)
        if bias:
            self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        if weight_norm:
            self.weight_g = nn.Parameter(w.flatten(1).norm(dim=1).view(-1, 1, 1))
            self.weight_v = nn.Parameter(w)

    def forward(self, x):
        raise RuntimeError("this module only holds parameters: WaveGlow.infer runs the layers in HIP")


def _weight_normed(mod) -> bool:
    return "weight_g" in mod._parameters


def _folded(mod) -> torch.Tensor:
    """g * v / ||v|| over dim 0, as weight_norm computes it; the plain weight once the norm is removed.  Folded on the host,
    wherever the parameters live: the norm's bits then do not depend on the device, so a module gives the same audio before
    and after remove_weightnorm, whether that ran before or after .cuda()."""
    if _weight_normed(mod):
        v = mod.weight_v.detach()
        return torch._weight_norm(v.cpu(), mod.weight_g.detach().cpu(), 0).to(v.device)
    return mod.weight.detach()


def _remove_weight_norm(mod):
    if not _weight_normed(mod):
        raise ValueError("weight_norm of 'weight' not found in {}".format(mod))
    if not isinstance(mod, _Conv):                  # torch's own module, from a checkpoint pickled by the reference
        return torch.nn.utils.remove_weight_norm(mod)
    w = _folded(mod)
    del mod._parameters["weight_g"], mod._parameters["weight_v"]
    mod.weight = nn.Parameter(w)                     # the reference's order after removal: bias, weight
    return mod


class _FlowFunction(torch.autograd.Function):
    """(z, log_s[0], .., log_s[n_flows-1]) from the folded fp32 tensors in the order ``WaveGlow._tensors(forward=True)`` lists
    them: t2_waveglow_train_forward, and t2_waveglow_backward for arbitrary upstream gradients (a missing one counts as zero).
    The backward returns one gradient per folded tensor, as views into one arena.  No host synchronisation on the stream, except
    under kernel_times.  ``keep`` is the caller's word on whether a backward can follow (grad mode on and a parameter requiring
    grad; ``needs_input_grad`` cannot tell, it ignores grad mode): without it nothing is kept and the plain t2_waveglow_forward runs
    on the same packed weights.  Upstream gradients are not materialised: an output the loss does not use reaches the driver as a
    null pointer, not as a tensor of zeros."""

    @staticmethod
    def forward(ctx, cfg, kernel_times, keep, mel, audio, *tensors):
        dev, f32 = mel.device, torch.float32
        (B, n_mel, T), N = mel.shape, audio.shape[1]
        need = bool(keep)
        ctx.set_materialize_grads(False)
        plan = L.waveglow_forward_plan(cfg, B, T, N)               # refuses N < n_group and N > (T - 1) * 256 + 1024, by value
        with torch.cuda.device(dev):
            ts = [t.detach().to(f32).contiguous() for t in tensors]
            mel, audio = mel.contiguous(), audio.contiguous()
            packed = torch.empty(plan.packed_bytes // 4, device=dev, dtype=f32)
            tp = (C.c_void_p * len(ts))(*[L.ptr(t) for t in ts])
            L.check(L.lib().t2_waveglow_pack(C.byref(cfg), tp, len(ts), L.ptr(packed), L.stream()))
            ws = torch.empty(plan.workspace_bytes // 4, device=dev, dtype=f32)
            z = torch.empty(B, cfg.n_group, plan.L, device=dev, dtype=f32)
            log_s = [torch.empty(B, t.shape[0] // 2, plan.L, device=dev, dtype=f32) for t in ts[2 + 6 + 4 * cfg.n_layers::7 + 4 * cfg.n_layers]]
            assert len(log_s) == cfg.n_flows and sum(t.shape[1] for t in log_s) == plan.n_log_s_rows
            table = (C.c_void_p * len(log_s))(*[L.ptr(t) for t in log_s])
            ms = (C.c_double * len(L.WAVEGLOW_FORWARD_KERNELS))() if kernel_times is not None else None
            a = L.WaveglowForwardArgs(B, T, n_mel, N, L.ptr(packed), None, L.ptr(mel), L.ptr(audio), L.ptr(ws), L.ptr(z), table, None, 1.0, None, None,
                                      None, ms)
            if need:
                bplan = L.waveglow_backward_plan(cfg, B, T, N)
                saved = torch.empty(bplan.saved_bytes // 4, device=dev, dtype=f32)
                L.check(L.lib().t2_waveglow_train_forward(C.byref(cfg), C.byref(L.WaveglowTrainForwardArgs(a, L.ptr(saved))), L.stream()))
                ctx.cfg, ctx.kernel_times, ctx.packed, ctx.saved, ctx.shape = cfg, kernel_times, packed, saved, (B, T, N)
                ctx.save_for_backward(mel, audio, *ts)
            else:
                L.check(L.lib().t2_waveglow_forward(C.byref(cfg), C.byref(a), L.stream()))
        if kernel_times is not None:
            kernel_times["forward"] = dict(zip(L.WAVEGLOW_FORWARD_KERNELS, ms))
        return (z, *log_s)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz, *dlog_s):
        cfg, (B, T, N) = ctx.cfg, ctx.shape
        mel, audio, *ts = ctx.saved_tensors
        dev, f32 = mel.device, torch.float32
        plan = L.waveglow_backward_plan(cfg, B, T, N)
        with torch.cuda.device(dev):
            ups = [None if g is None else g.to(f32).contiguous() for g in (dz, *dlog_s)]
            packed_bwd = torch.empty(plan.packed_bwd_bytes // 4, device=dev, dtype=f32)
            tp = (C.c_void_p * len(ts))(*[L.ptr(t) for t in ts])
            L.check(L.lib().t2_waveglow_pack_backward(C.byref(cfg), tp, len(ts), L.ptr(packed_bwd), L.stream()))
            ws = torch.empty(plan.workspace_bytes // 4, device=dev, dtype=f32)
            arena = torch.empty(plan.grad_floats, device=dev, dtype=f32)
            table = (C.c_void_p * cfg.n_flows)(*[L.ptr(g) for g in ups[1:]])
            ms = (C.c_double * len(L.WAVEGLOW_BACKWARD_KERNELS))() if ctx.kernel_times is not None else None
            a = L.WaveglowBackwardArgs(B, T, mel.shape[1], N, L.ptr(ctx.packed), L.ptr(packed_bwd), L.ptr(ctx.saved), L.ptr(mel), L.ptr(audio), L.ptr(ups[0]),
                                       table, L.ptr(ws), L.ptr(arena), ms)
            L.check(L.lib().t2_waveglow_backward(C.byref(cfg), C.byref(a), L.stream()))
        if ctx.kernel_times is not None:
            ctx.kernel_times["backward"] = dict(zip(L.WAVEGLOW_BACKWARD_KERNELS, ms))
            ctx.kernel_times["arena"] = arena
        offs = L.waveglow_grad_offsets(cfg, len(ts))
        assert offs[-1] + ts[-1].numel() == plan.grad_floats
        return (None, None, None, None, None, *[arena[o:o + t.numel()].view(t.shape) for o, t in zip(offs, ts)])


class Invertible1x1Conv(nn.Module):
    """Parameters of glow.py:62-80: ``conv.weight`` [c, c, 1], a random orthonormal matrix of determinant 1."""

    def __init__(self, c):
        super().__init__()
        self.conv = _Conv(c, c, 1, weight_norm=False, bias=False)
        W = torch.linalg.qr(torch.empty(c, c).normal_())[0]
        if torch.det(W) < 0:
            W[:, 0] = -1 * W[:, 0]
        self.conv.weight.data = W.view(c, c, 1).contiguous()

    def forward(self, z, reverse=False):
        raise RuntimeError("this module only holds parameters: WaveGlow.infer applies the inverse in HIP")


class WN(nn.Module):
    """Parameters of glow.py:105-151, registered in the reference's order."""

    def __init__(self, n_in_channels, n_mel_channels, n_layers, n_channels, kernel_size):
        super().__init__()
        assert kernel_size % 2 == 1
        assert n_channels % 2 == 0
        self.n_layers = n_layers
        self.n_channels = n_channels
        self.in_layers = nn.ModuleList()
        self.res_skip_layers = nn.ModuleList()
        self.start = _Conv(n_in_channels, n_channels, 1)
        # the reference starts `end` at zero, so that a fresh coupling is the identity
        self.end = _Conv(n_channels, 2 * n_in_channels, 1, weight_norm=False)
        self.end.weight.data.zero_()
        self.end.bias.data.zero_()
        self.cond_layer = _Conv(n_mel_channels, 2 * n_channels * n_layers, 1)
        for i in range(n_layers):
            self.in_layers.append(_Conv(n_channels, 2 * n_channels, kernel_size, dilation=2 ** i))
            self.res_skip_layers.append(_Conv(n_channels, 2 * n_channels if i < n_layers - 1 else n_channels, 1))

    def forward(self, forward_input):
        raise RuntimeError("this module only holds parameters: WaveGlow.infer runs the layers in HIP")


class WaveGlow(nn.Module):
    def __init__(self, n_mel_channels, n_flows, n_group, n_early_every, n_early_size, WN_config):
        super().__init__()
        assert n_group % 2 == 0
        L.waveglow_plan(L.waveglow_config(n_mel_channels, n_flows, n_group, n_early_every, n_early_size, WN_config), 1, 1)   # refuses here, by name
        self.upsample = _Conv(n_mel_channels, n_mel_channels, 1024, weight_norm=False, transposed=True, stride=256)
        self.n_flows = n_flows
        self.n_group = n_group
        self.n_early_every = n_early_every
        self.n_early_size = n_early_size
        self.WN = nn.ModuleList()
        self.convinv = nn.ModuleList()
        n_half = int(n_group / 2)
        n_remaining_channels = n_group
        for k in range(n_flows):
            if k % self.n_early_every == 0 and k > 0:
                n_half = n_half - int(self.n_early_size / 2)
                n_remaining_channels = n_remaining_channels - self.n_early_size
            self.convinv.append(Invertible1x1Conv(n_remaining_channels))
            self.WN.append(WN(n_half, n_mel_channels * n_group, **WN_config))
        self.n_remaining_channels = n_remaining_channels

    # ---- the cache of packed weights lives outside the pickled state and outside what __init__ sets, so that a module
    # unpickled from a checkpoint (no __init__) works too
    def __getstate__(self):
        state = dict(self.__dict__)
        for name in _CACHES:
            state.pop(name, None)
        return state

    def _drop_caches(self):
        for name in _CACHES:
            self.__dict__.pop(name, None)

    def _config(self) -> L.WaveglowConfig:
        wn = self.WN[0]
        if not hasattr(wn, "cond_layer"):
            raise RuntimeError("WaveGlow: this module keeps one cond_layer per layer (WN.cond_layers), the older layout of the "
                               "reference's waveglow/glow.py; convert it to the single cond_layer of glow.py:132 first")
        k = wn.in_layers[0].kernel_size
        return L.waveglow_config(self.upsample.in_channels, self.n_flows, self.n_group, self.n_early_every, self.n_early_size,
                                 dict(n_layers=wn.n_layers, n_channels=wn.n_channels, kernel_size=k[0] if isinstance(k, (tuple, list)) else k))

    def trainable(self, on=True):
        """Opt in to training: ``model((mel, audio))`` then runs the forward that keeps what the backward reads, and
        ``WaveGlowLoss(sigma)(outputs).backward()`` leaves ``.grad`` on every parameter.  A plain attribute, read with
        ``getattr(..., False)``: a module pickled by the reference lacks it and stays refused.  Returns self."""
        self._trainable = bool(on)
        return self

    def forward(self, forward_input):
        if not getattr(self, "_trainable", False):
            raise RuntimeError("WaveGlow is inference only here: forward (the training direction, audio -> z) has no backward, so it stays "
                               "refused; call infer, or analyze / nll for the values of that direction under torch.no_grad()")
        return self._train_forward(forward_input)

    def _train_tensors(self):
        """``_tensors(forward=True)`` as differentiable fp32 tensors: the weight norm is folded on the device by torch's own
        ``_weight_norm``, so autograd carries a folded tensor's gradient on to ``weight_g`` / ``weight_v`` (or ``weight``)."""
        fold = lambda m: torch._weight_norm(m.weight_v, m.weight_g, 0) if _weight_normed(m) else m.weight
        out = [self.upsample.weight, self.upsample.bias]
        for wn, inv in zip(self.WN, self.convinv):
            out += [fold(wn.start), wn.start.bias, fold(wn.cond_layer), wn.cond_layer.bias]
            for l in wn.in_layers:
                out += [fold(l), l.bias]
            for l in wn.res_skip_layers:
                out += [fold(l), l.bias]
            out += [wn.end.weight, wn.end.bias, inv.conv.weight.squeeze(-1)]
        return out

    def _train_forward(self, forward_input, kernel_times=None):
        """The reference's ``forward`` (glow.py:207-249) with a backward.  Two differences from ``analyze``: the weight norm is
        folded on the device, so z may differ from analyze's (host fold) in the last bits; and, the parameters changing every
        step, the weights are packed on every call into a buffer of their own -- the ``_key()`` cache and ``_packed`` /
        ``_packed_fwd`` are neither read nor written.  kernel_times: a dict that receives ``forward`` and ``backward``, the time
        per kind of kernel (synchronises; for scripts/time_waveglow_train.py)."""
        spect, audio = forward_input
        who = "WaveGlow.forward"
        dev = self.upsample.weight.device
        if dev.type != "cuda" or not (spect.is_cuda and audio.is_cuda):
            raise RuntimeError(f"{who}: the parameters, the mel and the audio must live on the GPU (the product path has no CPU fallback)")
        if torch.is_grad_enabled() and spect.requires_grad:
            raise RuntimeError(f"{who}: the mel requires grad, but the gradient with respect to the mel is not built")
        if torch.is_grad_enabled() and audio.requires_grad:
            raise RuntimeError(f"{who}: the audio requires grad, but the gradient with respect to the audio is not built")
        cfg = self._config()
        if spect.dim() != 3 or spect.shape[1] != cfg.n_mel_channels:
            raise RuntimeError(f"{who}: expected a mel of shape [B, {cfg.n_mel_channels}, T] (upsample takes "
                               f"{cfg.n_mel_channels} channels), got {tuple(spect.shape)}")
        if audio.dim() != 2 or audio.shape[0] != spect.shape[0]:
            raise RuntimeError(f"{who}: expected audio of shape [B, N] with B = {spect.shape[0]}, got {tuple(audio.shape)}")
        if spect.dtype != torch.float32 or audio.dtype != torch.float32 or any(p.dtype != torch.float32 for p in self.parameters()):
            raise RuntimeError(f"{who}: the mel, the audio and the parameters must be float32 (fp16 and amp are not built)")
        if torch.is_autocast_enabled():
            raise RuntimeError(f"{who}: autocast is on, but fp16 and amp are not built")
        if audio.device != spect.device or dev != spect.device:
            raise RuntimeError(f"{who}: the mel is on {spect.device}, the audio on {audio.device}, the parameters on {dev}")
        B, L_ = spect.shape[0], audio.shape[1] // cfg.n_group
        tensors = self._train_tensors()
        keep = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        outs = _FlowFunction.apply(cfg, kernel_times, keep, spect.detach(), audio.detach(), *tensors)
        logdet = [B * L_ * torch.logdet(inv.conv.weight.squeeze(-1)) for inv in self.convinv]            # glow.py:100, torch's own autograd
        return outs[0], list(outs[1:]), logdet

    @staticmethod
    def remove_weightnorm(model):
        waveglow = model
        for wn in waveglow.WN:
            _remove_weight_norm(wn.start)
            for l in list(wn.in_layers) + list(wn.res_skip_layers):
                _remove_weight_norm(l)
            _remove_weight_norm(wn.cond_layer)
        waveglow._drop_caches()
        return waveglow

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._drop_caches()
        return out

    def _apply(self, fn, *args, **kwargs):               # .to() / .cuda() / .float()
        out = super()._apply(fn, *args, **kwargs)
        self._drop_caches()
        return out

    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _tensors(self, forward=False):
        """The folded weights in the order t2_waveglow_pack takes them; forward: W_k itself where inference has its inverse."""
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        out = [f32(self.upsample.weight), f32(self.upsample.bias)]
        for wn, inv in zip(self.WN, self.convinv):
            out += [f32(_folded(wn.start)), f32(wn.start.bias), f32(_folded(wn.cond_layer)), f32(wn.cond_layer.bias)]
            for l in wn.in_layers:
                out += [f32(_folded(l)), f32(l.bias)]
            for l in wn.res_skip_layers:
                out += [f32(_folded(l)), f32(l.bias)]
            W = inv.conv.weight.detach().squeeze(-1)
            out += [f32(wn.end.weight), f32(wn.end.bias), f32(W) if forward else f32(W.float().inverse())]     # glow.py:91
        return out

    def repack(self):
        """Fold, invert and pack the weights again (and, once analyze / nll have run, their buffer too).  infer(), analyze() and
        nll() do this by themselves after load_state_dict, remove_weightnorm, .to() and in-place updates that autograd sees; call
        it after editing parameters behind autograd's back (``.data``)."""
        forward = getattr(self, "_packed_fwd", None) is not None
        self._pack(False)
        if forward:
            self._pack(True)
        return self

    def _pack(self, forward):
        """One packed buffer: inference's (the inverse mixes) or, forward, the analysis direction's (W_k itself, and log|det W_k|)."""
        dev = self.upsample.weight.device
        if dev.type != "cuda":
            raise RuntimeError("WaveGlow: the parameters must live on the GPU (the product path has no CPU fallback)")
        cfg = self._config()
        plan = L.waveglow_plan(cfg, 1, 1)
        with torch.no_grad():
            ts = self._tensors(forward)
        packed = torch.empty(plan.packed_bytes // 4, device=dev, dtype=torch.float32)
        tp = (C.c_void_p * len(ts))(*[L.ptr(t) for t in ts])
        with torch.cuda.device(dev):
            L.check(L.lib().t2_waveglow_pack(C.byref(cfg), tp, len(ts), L.ptr(packed), L.stream()))
            if forward:
                logdet = torch.empty(cfg.n_flows, device=dev, dtype=torch.float32)
                L.check(L.lib().t2_waveglow_logdet(C.byref(cfg), L.ptr(packed), L.ptr(logdet), L.stream()))
        if forward:
            self._packed_fwd, self._logdet_fwd, self._packed_fwd_key = packed, logdet, self._key()
        else:
            self._packed, self._packed_key = packed, self._key()

    def infer(self, spect, sigma=1.0, noise=None):
        """mel [B, n_mel_channels, T], fp32, on the GPU -> audio [B, T * 256] (glow.py:251-293).  The noise planes are drawn
        on the device in the reference's order -- [B, n_remaining_channels, L] first, then one [B, n_early_size, L] per early
        flow, k descending -- also when sigma == 0, so that a seeded script consumes the generator as the reference does.
        ``noise`` (an addition) supplies them instead."""
        return self.infer_debug(spect, sigma, noise)[0]

    def infer_debug(self, spect, sigma=1.0, noise=None, debug=False, kernel_times=False):
        """infer, returning (audio, info).  debug: info holds ``spect`` [B, n_mel*G, L] (the upsampled, regrouped mel) and
        ``flow_audio`` [B, G, L] (the tensor after the last flow).  kernel_times: info holds ``kernel_ms``, the time spent in
        every kind of kernel (each launch bracketed by events: slower than a plain call)."""
        if not spect.is_cuda:
            raise RuntimeError("WaveGlow.infer: the mel must live on the GPU, as the reference's torch.cuda.FloatTensor noise "
                               "requires (the product path has no CPU fallback)")
        if torch.is_grad_enabled() and (spect.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("WaveGlow.infer is inference only: grad mode is on and the mel or the parameters require grad; "
                               "call it under torch.no_grad(), as inference.py:166 does")
        cfg = self._config()
        if spect.dim() != 3 or spect.shape[1] != cfg.n_mel_channels:
            raise RuntimeError(f"WaveGlow.infer: expected a mel of shape [B, {cfg.n_mel_channels}, T] (upsample takes "
                               f"{cfg.n_mel_channels} channels), got {tuple(spect.shape)}")
        if spect.dtype != torch.float32:
            raise RuntimeError(f"WaveGlow.infer: the mel must be float32, got {spect.dtype} (fp16 inference is not built)")
        packed = getattr(self, "_packed", None)
        if packed is None or packed.device != spect.device or getattr(self, "_packed_key", None) != self._key():
            self.repack()
            packed = self._packed
            if packed.device != spect.device:
                raise RuntimeError(f"WaveGlow.infer: the mel is on {spect.device}, the parameters on {packed.device}")
        B, n_mel, T = spect.shape
        plan = L.waveglow_plan(cfg, B, T)
        shapes = [(B, plan.n_remaining_channels, plan.L)] + [(B, cfg.n_early_size, plan.L)] * (plan.n_noise_planes - 1)
        with torch.cuda.device(spect.device):
            if noise is None:
                noise = [torch.empty(s, device=spect.device, dtype=torch.float32).normal_() for s in shapes]
            else:
                noise = list(noise)
                if len(noise) != len(shapes):
                    raise RuntimeError(f"WaveGlow.infer: {len(noise)} noise planes given, the model draws {len(shapes)}")
                for z, s in zip(noise, shapes):
                    if tuple(z.shape) != s or z.dtype != torch.float32 or z.device != spect.device:
                        raise RuntimeError(f"WaveGlow.infer: a noise plane is {tuple(z.shape)} {z.dtype} on {z.device}, "
                                           f"expected {s} float32 on {spect.device}")
                noise = [z.detach().contiguous() for z in noise]
            mel = spect.detach().contiguous()
            ws = torch.empty(plan.workspace_bytes // 4, device=spect.device, dtype=torch.float32)
            audio = torch.empty(B, plan.out_len, device=spect.device, dtype=torch.float32)
            info = {}
            if debug:
                info["spect"] = torch.empty(B, n_mel * cfg.n_group, plan.L, device=spect.device, dtype=torch.float32)
                info["flow_audio"] = torch.empty(B, cfg.n_group, plan.L, device=spect.device, dtype=torch.float32)
            ms = (C.c_double * len(L.WAVEGLOW_KERNELS))() if kernel_times else None
            planes = (C.c_void_p * len(noise))(*[L.ptr(z) for z in noise])
            a = L.WaveglowInferArgs(B, T, n_mel, L.ptr(packed), L.ptr(mel), planes, len(noise), float(sigma), L.ptr(ws), L.ptr(audio),
                                    L.ptr(info.get("spect")), L.ptr(info.get("flow_audio")), ms)
            L.check(L.lib().t2_waveglow_infer(C.byref(cfg), C.byref(a), L.stream()))
        if kernel_times:
            info["kernel_ms"] = dict(zip(L.WAVEGLOW_KERNELS, ms))
        return audio, info

    # ---- the analysis direction: audio -> z, log_s, log det W (glow.py:207-249), values only
    def analyze(self, forward_input):
        """``(spect [B, n_mel_channels, T], audio [B, N])``, fp32 on the GPU -> ``(z, log_s_list, log_det_W_list)`` as the
        reference's ``forward`` returns them: z [B, n_group, L] with L = N // n_group (early outputs first, k ascending, then the
        last flow's audio; a tail of N % n_group samples is dropped, as ``unfold`` drops it), log_s_list[k] [B, n_half_k, L] and
        log_det_W_list[k] = B * L * logdet(W_k), a 0-dim tensor.  N may reach (T - 1) * 256 + 1024, the length of the transposed
        conv's output.  Values only: no gradient flows, which is why ``forward`` still refuses."""
        return self._forward_direction(forward_input, "analyze", want_outputs=True)[:3]

    def nll(self, spect, audio, sigma=1.0, per_item=False):
        """``WaveGlowLoss(sigma)(analyze((spect, audio)))`` as a device scalar, from sums the kernels form in fp64 in a fixed
        order; no log_s tensor is written.  per_item: [B], every item's own mean negative log-likelihood per sample (their
        mean is the scalar)."""
        out = self._forward_direction((spect, audio), "nll", want_outputs=False, sigma=sigma)
        return out[4] if per_item else out[3]

    def analyze_debug(self, forward_input, sigma=1.0, kernel_times=False):
        """analyze, returning (z, log_s_list, log_det_W_list, info): info holds ``loss``, ``nll_item`` [B] and ``sums``
        [B, n_flows + 1] fp64 (per item the sum of every log_s[k], then the sum of z^2) and, kernel_times, ``kernel_ms``."""
        z, log_s, logdet, loss, item, sums, ms = self._forward_direction(forward_input, "analyze", want_outputs=True, sigma=sigma, want_sums=True,
                                                                         kernel_times=kernel_times)
        info = dict(loss=loss, nll_item=item, sums=sums)
        if kernel_times:
            info["kernel_ms"] = ms
        return z, log_s, logdet, info

    def _forward_direction(self, forward_input, who, want_outputs, sigma=1.0, want_sums=None, kernel_times=False):
        spect, audio = forward_input
        who = "WaveGlow." + who
        if not (spect.is_cuda and audio.is_cuda):
            raise RuntimeError(f"{who}: the mel and the audio must live on the GPU (the product path has no CPU fallback)")
        if torch.is_grad_enabled() and (spect.requires_grad or audio.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError(f"{who} computes values only, the backward is not built: grad mode is on and the inputs or the "
                               "parameters require grad; call it under torch.no_grad()")
        cfg = self._config()
        if spect.dim() != 3 or spect.shape[1] != cfg.n_mel_channels:
            raise RuntimeError(f"{who}: expected a mel of shape [B, {cfg.n_mel_channels}, T] (upsample takes "
                               f"{cfg.n_mel_channels} channels), got {tuple(spect.shape)}")
        if audio.dim() != 2 or audio.shape[0] != spect.shape[0]:
            raise RuntimeError(f"{who}: expected audio of shape [B, N] with B = {spect.shape[0]}, got {tuple(audio.shape)}")
        if spect.dtype != torch.float32 or audio.dtype != torch.float32:
            raise RuntimeError(f"{who}: the mel and the audio must be float32, got {spect.dtype} and {audio.dtype} (fp16 is not built)")
        if audio.device != spect.device:
            raise RuntimeError(f"{who}: the mel is on {spect.device}, the audio on {audio.device}")
        want_sums = (not want_outputs) if want_sums is None else want_sums
        if want_sums and not float(sigma) > 0.0:
            raise RuntimeError(f"{who}: sigma={sigma} must be positive")
        packed = getattr(self, "_packed_fwd", None)
        if packed is None or packed.device != spect.device or getattr(self, "_packed_fwd_key", None) != self._key():
            self._pack(True)
            packed = self._packed_fwd
            if packed.device != spect.device:
                raise RuntimeError(f"{who}: the mel is on {spect.device}, the parameters on {packed.device}")
        (B, n_mel, T), N = spect.shape, audio.shape[1]
        plan = L.waveglow_forward_plan(cfg, B, T, N)               # refuses N < n_group and N > (T - 1) * 256 + 1024, by value
        dev, f32 = spect.device, torch.float32
        with torch.cuda.device(dev):
            mel, wave = spect.detach().contiguous(), audio.detach().contiguous()
            ws = torch.empty(plan.workspace_bytes // 4, device=dev, dtype=f32)
            z = log_s = logdet = loss = item = sums = table = None
            if want_outputs:
                z = torch.empty(B, cfg.n_group, plan.L, device=dev, dtype=f32)
                log_s = [torch.empty(B, inv.conv.weight.shape[0] // 2, plan.L, device=dev, dtype=f32) for inv in self.convinv]
                assert sum(t.shape[1] for t in log_s) == plan.n_log_s_rows
                table = (C.c_void_p * len(log_s))(*[L.ptr(t) for t in log_s])
                logdet = torch.empty(cfg.n_flows, device=dev, dtype=f32)
            if want_sums:
                loss, item = torch.empty((), device=dev, dtype=f32), torch.empty(B, device=dev, dtype=f32)
                sums = torch.empty(B, cfg.n_flows + 1, device=dev, dtype=torch.float64)
            ms = (C.c_double * len(L.WAVEGLOW_FORWARD_KERNELS))() if kernel_times else None
            a = L.WaveglowForwardArgs(B, T, n_mel, N, L.ptr(packed), L.ptr(self._logdet_fwd), L.ptr(mel), L.ptr(wave), L.ptr(ws), L.ptr(z), table,
                                      L.ptr(logdet), float(sigma), L.ptr(sums), L.ptr(item), L.ptr(loss), ms)
            L.check(L.lib().t2_waveglow_forward(C.byref(cfg), C.byref(a), L.stream()))
        return (z, log_s, None if logdet is None else list(logdet.unbind(0)), loss, item, sums,
                dict(zip(L.WAVEGLOW_FORWARD_KERNELS, ms)) if kernel_times else None)
