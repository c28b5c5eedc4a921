"""Drop-in for the reference's ``hifigan_infer.hifigan_model.Generator`` (hifigan_model.py:75-124) on the MI355X.

The modules below only hold parameters, under the names and shapes the reference's checkpoints use; ``Generator.forward``
hands the folded weights to the HIP library (csrc/vocoder.hip) once, packed into the order its kernels read, and then
runs the whole generator through ``t2_hifigan_forward``.  So the reference's three lines work verbatim::

    generator = Generator(h)
    generator.load_state_dict(state_dict_g['generator'])
    generator.eval(); generator.remove_weight_norm()
    audio = generator(mel)            # mel [B, 80, T] fp32 on the GPU -> [B, 1, T * prod(upsample_rates)]

Inference only unless ``Generator.trainable()`` opts in; always fp32 (``set_precision`` does not reach the vocoder); no CPU
path.  The adversarial side is below: ``DiscriminatorP`` / ``MultiPeriodDiscriminator`` (hifigan_model.py:127-187) in HIP
(csrc/vocoder_disc.hip) and ``feature_loss`` / ``discriminator_loss`` / ``generator_loss`` (:250-281); ``MultiScaleDiscriminator`` is
not built.  Opted in, ``forward`` keeps every conv's pre-activation input and registers one autograd node whose
backward is HIP (csrc/vocoder_bwd.hip)::

    gen = Generator(h).cuda().trainable()
    y_hat = gen(mel)                                   # [B, 1, T * prod(rates)], carries grad
    loss = F.l1_loss(mel_spectrogram_from_audio(y_hat.squeeze(1), differentiable=True), mel_target) * 45
    loss.backward()                                    # .grad on every bias / weight_g / weight_v (or weight, once folded)"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import nn

from .. import _lib as L
from .hifigan_utils import get_padding

LRELU_SLOPE = 0.1


class _WNConv(nn.Module):
    """Parameters of a weight-normed Conv1d / ConvTranspose1d as torch.nn.utils.weight_norm leaves them: ``bias``,
    ``weight_g`` [shape[0], 1, 1], ``weight_v``; after remove_weight_norm(): ``bias``, ``weight``.  Conv1d weights are
    [Cout, Cin, k], ConvTranspose1d weights [Cin, Cout, k], so the norm runs over dim 0 = the input channels there."""

    def __init__(self, cin, cout, k, transposed=False, dilation=1, stride=1, std=0.01):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, k
        self.transposed, self.dilation, self.stride = transposed, dilation, stride
        shape = (cin, cout, k) if transposed else (cout, cin, k)
        fan_in = shape[1] * k
        v = torch.empty(shape)
        if std is None:                                  # conv_pre keeps torch's default initialisation
            nn.init.kaiming_uniform_(v, a=math.sqrt(5))
        else:                                            # init_weights, hifigan_utils.py:22-25
            v.normal_(0.0, std)
        bound = 1.0 / math.sqrt(fan_in)
        self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(-1, 1, 1))
        self.weight_v = nn.Parameter(v)

    @property
    def weight_normed(self) -> bool:
        return "weight_g" in self._parameters

    def folded_weight(self) -> torch.Tensor:
        """g * v / ||v|| over dim 0, as weight_norm computes it; the plain weight once the norm is removed."""
        if self.weight_normed:
            return torch._weight_norm(self.weight_v.detach(), self.weight_g.detach(), 0)
        return self.weight.detach()

    def remove_weight_norm(self):
        if not self.weight_normed:
            raise ValueError("weight_norm of 'weight' not found in {}".format(self))
        w = self.folded_weight()
        del self._parameters["weight_g"], self._parameters["weight_v"]
        self.weight = nn.Parameter(w)

    def forward(self, x):
        raise RuntimeError("this module only holds parameters: Generator.forward runs the layers in HIP")


def _resconv(channels, k, d):
    assert get_padding(k, d) * 2 == k * d - d
    return _WNConv(channels, channels, k, dilation=d)


class _GeneratorFunction(torch.autograd.Function):
    """audio from the mel and the folded fp32 tensors (weight, bias per layer, in ``Generator._layers()`` order).  The weights are
    packed here, on every call, into buffers of the call's own (the forward pack and the data-gradient packs): the parameters
    change between calls, and an optimizer that writes through raw pointers (``optim.FusedAdam``) leaves no trace in a parameter's
    version.  t2_hifigan_forward_train, then t2_hifigan_backward for an arbitrary gradient on the audio.  The backward returns one
    gradient per folded tensor, as views into one arena, and the mel's where it is asked for; where no folded tensor asks for a
    gradient the weight gradients are not launched and the arena is not allocated."""

    @staticmethod
    def forward(ctx, cfg, mel, *tensors):
        dev, f32 = mel.device, torch.float32
        B, n_mel, T = mel.shape
        plan = L.hifigan_train_plan(cfg, B, T)
        n = plan.n_layers
        with torch.cuda.device(dev):
            ts = [t.detach().to(f32).contiguous() for t in tensors]
            mel = mel.detach().contiguous()
            packed = torch.empty(plan.packed_bytes // 4, device=dev, dtype=f32)
            packed_bwd = torch.empty(plan.packed_bwd_bytes // 4, device=dev, dtype=f32)
            wp = (C.c_void_p * n)(*[L.ptr(w) for w in ts[0::2]])
            bp = (C.c_void_p * n)(*[L.ptr(b) for b in ts[1::2]])
            L.check(L.lib().t2_hifigan_pack(C.byref(cfg), wp, bp, n, L.ptr(packed), L.stream()))
            L.check(L.lib().t2_hifigan_pack_backward(C.byref(cfg), wp, n, L.ptr(packed_bwd), L.stream()))
            tape = torch.empty(plan.tape_bytes // 4, device=dev, dtype=f32)
            audio = torch.empty(B, 1, plan.out_len, device=dev, dtype=f32)
            a = L.HifiganTrainFwdArgs(B, T, n_mel, L.ptr(packed), L.ptr(mel), L.ptr(tape), L.ptr(audio))
            L.check(L.lib().t2_hifigan_forward_train(C.byref(cfg), C.byref(a), L.stream()))
        ctx.cfg, ctx.packed, ctx.packed_bwd, ctx.tape = cfg, packed, packed_bwd, tape
        ctx.shapes = [t.shape for t in tensors]
        ctx.save_for_backward(mel, audio)
        return audio

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_audio):
        cfg = ctx.cfg
        mel, audio = ctx.saved_tensors
        dev, f32 = mel.device, torch.float32
        B, n_mel, T = mel.shape
        plan = L.hifigan_train_plan(cfg, B, T)
        want_w = any(ctx.needs_input_grad[2:])
        with torch.cuda.device(dev):
            d_audio = d_audio.to(f32).contiguous()
            ws = torch.empty(plan.workspace_bytes // 4, device=dev, dtype=f32)
            arena = torch.empty(plan.grad_floats, device=dev, dtype=f32) if want_w else None
            d_mel = torch.empty_like(mel) if ctx.needs_input_grad[1] else None
            a = L.HifiganBwdArgs(B, T, n_mel, L.ptr(ctx.packed), L.ptr(ctx.packed_bwd), L.ptr(mel), L.ptr(ctx.tape), L.ptr(audio), L.ptr(d_audio),
                                 L.ptr(ws), L.ptr(arena), L.ptr(d_mel))
            L.check(L.lib().t2_hifigan_backward(C.byref(cfg), C.byref(a), L.stream()))
        grads = [None] * len(ctx.shapes)
        if want_w:
            woff, boff = L.hifigan_grad_offsets(cfg, plan.n_layers)
            for i in range(plan.n_layers):
                ws_, bs_ = ctx.shapes[2 * i], ctx.shapes[2 * i + 1]
                grads[2 * i], grads[2 * i + 1] = arena[woff[i]:woff[i] + ws_.numel()].view(ws_), arena[boff[i]:boff[i] + bs_.numel()].view(bs_)
        return (None, d_mel, *grads)


class ResBlock1(nn.Module):
    """Parameters of hifigan_model.py:11-33."""

    def __init__(self, h, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        self.h = h
        self.convs1 = nn.ModuleList([_resconv(channels, kernel_size, d) for d in dilation])
        self.convs2 = nn.ModuleList([_resconv(channels, kernel_size, 1) for _ in dilation])

    def layers(self):
        return list(self.convs1) + list(self.convs2)

    def remove_weight_norm(self):
        for l in self.layers():
            l.remove_weight_norm()


class ResBlock2(nn.Module):
    """Parameters of hifigan_model.py:51-61."""

    def __init__(self, h, channels, kernel_size=3, dilation=(1, 3)):
        super().__init__()
        self.h = h
        self.convs = nn.ModuleList([_resconv(channels, kernel_size, d) for d in dilation])

    def layers(self):
        return list(self.convs)

    def remove_weight_norm(self):
        for l in self.layers():
            l.remove_weight_norm()


class Generator(nn.Module):
    def __init__(self, h):
        super().__init__()
        self.h = h
        self.num_kernels = len(h.resblock_kernel_sizes)
        self.num_upsamples = len(h.upsample_rates)
        self._cfg = L.hifigan_config(h)
        L.hifigan_plan(self._cfg, 1, 1)                  # refuses an unsupported configuration here, by name
        c0 = h.upsample_initial_channel
        self.conv_pre = _WNConv(80, c0, 7, std=None)
        resblock = ResBlock1 if str(h.resblock) == "1" else ResBlock2
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            self.ups.append(_WNConv(c0 // (2 ** i), c0 // (2 ** (i + 1)), k, transposed=True, stride=u))
        self.resblocks = nn.ModuleList()
        for i in range(len(self.ups)):
            ch = c0 // (2 ** (i + 1))
            for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
                self.resblocks.append(resblock(h, ch, k, d))
        self.conv_post = _WNConv(ch, 1, 7)
        self.upsample_factor = math.prod(int(u) for u in h.upsample_rates)
        self._packed = None
        self._packed_key = None

    # ---- the order t2_hifigan_pack takes the layers in: the order of the state dict
    def _layers(self):
        out = [self.conv_pre] + list(self.ups)
        for rb in self.resblocks:
            out += rb.layers()
        return out + [self.conv_post]

    def remove_weight_norm(self):
        for l in self.ups:
            l.remove_weight_norm()
        for l in self.resblocks:
            l.remove_weight_norm()
        self.conv_pre.remove_weight_norm()
        self.conv_post.remove_weight_norm()
        self._packed = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._packed = None
        return out

    def _apply(self, fn, *args, **kwargs):               # .to() / .cuda() / .float()
        out = super()._apply(fn, *args, **kwargs)
        self._packed = None
        return out

    def trainable(self, on=True):
        """Opt in to training: ``forward`` then keeps what the backward reads whenever grad mode is on and a parameter or the mel
        requires grad, and ``loss.backward()`` leaves ``.grad`` on every parameter (and on the mel, if it asks).  A plain
        attribute, read with ``getattr(..., False)``.  ``trainable(False)`` restores the inference-only behaviour.  Returns self."""
        self._trainable = bool(on)
        return self

    def _train_forward(self, x, lengths):
        """The generator with a backward.  The weight norm is folded on the device by torch's own ``_weight_norm``, so autograd carries a
        folded tensor's gradient on to ``weight_g`` / ``weight_v`` (or ``weight``).  The parameters changing every step, the folded
        tensors are packed on every call into buffers of the call's own (as ``WaveGlow._train_forward`` does): the ``_key()`` cache is
        not read, and it is dropped, so that the next inference call packs the parameters as they then are -- also after an
        optimizer that writes through raw pointers and bumps no version (``optim.FusedAdam``)."""
        who = "hifigan Generator"
        if lengths is not None:
            raise RuntimeError(f"{who}: lengths= together with a gradient is not built: training runs on fixed-length segments; "
                               "call it under torch.no_grad() for a ragged batch")
        if not x.is_cuda:
            raise RuntimeError(f"{who}: the mel must live on the GPU (the product path has no CPU fallback)")
        if x.dim() != 3:
            raise RuntimeError(f"{who}: expected a mel of shape [B, 80, T], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"{who}: the mel must be float32, got {x.dtype}")
        layers = self._layers()
        if layers[0].bias.device != x.device:
            raise RuntimeError(f"{who}: the mel is on {x.device}, the parameters on {layers[0].bias.device}")
        tensors = []
        for l in layers:
            tensors += [torch._weight_norm(l.weight_v, l.weight_g, 0) if l.weight_normed else l.weight, l.bias]
        self._packed = None
        return _GeneratorFunction.apply(self._cfg, x, *tensors)

    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def repack(self):
        """Fold and pack the weights again.  forward() does this by itself after load_state_dict, remove_weight_norm, .to()
        and in-place updates that autograd sees; call it after editing parameters behind autograd's back (``.data``)."""
        layers = self._layers()
        dev = layers[0].bias.device
        if dev.type != "cuda":
            raise RuntimeError("hifigan Generator: the parameters must live on the GPU (the product path has no CPU fallback)")
        plan = L.hifigan_plan(self._cfg, 1, 1)
        with torch.no_grad():
            ws = [l.folded_weight().to(torch.float32).contiguous() for l in layers]
            bs = [l.bias.detach().to(torch.float32).contiguous() for l in layers]
        packed = torch.empty(plan.packed_bytes // 4, device=dev, dtype=torch.float32)
        n = len(layers)
        wp = (C.c_void_p * n)(*[L.ptr(w) for w in ws])
        bp = (C.c_void_p * n)(*[L.ptr(b) for b in bs])
        with torch.cuda.device(dev):
            L.check(L.lib().t2_hifigan_pack(C.byref(self._cfg), wp, bp, n, L.ptr(packed), L.stream()))
        self._packed, self._packed_key = packed, self._key()
        return self

    def forward(self, x, return_pre_tanh=False, lengths=None):
        """mel [B, 80, T], fp32, on the GPU -> audio [B, 1, T * prod(upsample_rates)].  return_pre_tanh=True (a debug output,
        used by the tests) also returns conv_post's output before the tanh, same shape.
        lengths (an addition): per-item frame counts of a padded batch, in the convention of stft.log_mel: Python ints, checked
        here against [0, T], or an int32 device tensor [B], which is not read back and is clamped to [0, T] by the kernels.
        Item b is then computed as mel[b, :, :lengths[b]] alone would be, with the same bits; what the mel holds behind its
        length is never read, audio (and pre) are zero behind lengths[b] * prod(upsample_rates), and the result is
        (audio, sample_lengths) or (audio, pre, sample_lengths), sample_lengths an int32 device tensor [B]."""
        if getattr(self, "_trainable", False) and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if return_pre_tanh:
                raise RuntimeError("hifigan Generator: return_pre_tanh is a debug output of the inference path; it has no gradient")
            return self._train_forward(x, lengths)
        if not x.is_cuda:
            raise RuntimeError("hifigan Generator: the mel must live on the GPU (the product path has no CPU fallback)")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("hifigan Generator is inference only: the input requires grad and grad mode is on; "
                               "call it under torch.no_grad() or detach the mel")
        if x.dim() != 3:
            raise RuntimeError(f"hifigan Generator: expected a mel of shape [B, 80, T], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"hifigan Generator: the mel must be float32, got {x.dtype}")
        if self._packed is None or self._packed.device != x.device or self._packed_key != self._key():
            self.repack()
            if self._packed.device != x.device:
                raise RuntimeError(f"hifigan Generator: the mel is on {x.device}, the parameters on {self._packed.device}")
        B, n_mel, T = x.shape
        mel = x.detach().contiguous()
        plan = L.hifigan_plan(self._cfg, B, T)
        if lengths is not None:
            lengths = L.lengths_arg("hifigan Generator", lengths, B, T, x.device)
        with torch.cuda.device(x.device):
            ws = torch.empty(plan.workspace_bytes // 4, device=x.device, dtype=torch.float32)
            audio = torch.empty(B, 1, plan.out_len, device=x.device, dtype=torch.float32)
            pre = torch.empty_like(audio) if return_pre_tanh else None
            if lengths is None:
                a = L.HifiganFwdArgs(B, T, n_mel, L.ptr(self._packed), L.ptr(mel), L.ptr(ws), L.ptr(audio), L.ptr(pre))
                L.check(L.lib().t2_hifigan_forward(C.byref(self._cfg), C.byref(a), L.stream()))
                return (audio, pre) if return_pre_tanh else audio
            sample_lengths = torch.empty(B, device=x.device, dtype=torch.int32)
            a = L.HifiganRaggedArgs(B, T, n_mel, L.ptr(self._packed), L.ptr(mel), L.ptr(ws), L.ptr(audio), L.ptr(pre), L.ptr(lengths),
                                    L.ptr(sample_lengths))
            L.check(L.lib().t2_hifigan_forward_ragged(C.byref(self._cfg), C.byref(a), L.stream()))
        return (audio, pre, sample_lengths) if return_pre_tanh else (audio, sample_lengths)


# ----------------------------------------------------------------------------------------------------------------------
# the multi-period discriminator and the GAN losses
# ----------------------------------------------------------------------------------------------------------------------
_MPD_WIDTHS = (1, 32, 128, 512, 1024, 1024, 1)
_MSD_NOT_BUILT = ("only the multi-period discriminator's own convolutions are built (kernel_size=5, stride=3, weight norm); "
                  "the multi-scale discriminator (MultiScaleDiscriminator / DiscriminatorS, spectral norm) is not built")


class _WNConv2d(nn.Module):
    """Parameters of a weight-normed ``Conv2d(cin, cout, (k, 1))`` as torch.nn.utils.weight_norm leaves them: ``bias``,
    ``weight_g`` [cout, 1, 1, 1], ``weight_v`` [cout, cin, k, 1], initialised by Conv2d's defaults (the reference applies no
    init_weights to the discriminators)."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, (k, 1)
        v = torch.empty(cout, cin, k, 1)
        nn.init.kaiming_uniform_(v, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(cin * k)
        self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
        self.weight_v = nn.Parameter(v)

    def forward(self, x):
        raise RuntimeError("this module only holds parameters: DiscriminatorP.forward runs the layers in HIP")


def _mpd_launch(period, audio, tensors, backward_pack):
    """Packs the folded tensors (weight, bias per conv) and runs t2_hifigan_mpd_forward: the six feature maps, and the packs."""
    dev, f32 = audio.device, torch.float32
    B, _, T = audio.shape
    plan = L.hifigan_mpd_plan(period, B, T)
    n = L.HIFIGAN_MPD_LAYERS
    with torch.cuda.device(dev):
        ts = [t.detach().to(f32).contiguous() for t in tensors]
        wp = (C.c_void_p * n)(*[L.ptr(w) for w in ts[0::2]])
        bp = (C.c_void_p * n)(*[L.ptr(b) for b in ts[1::2]])
        packed = torch.empty(plan.packed_bytes // 4, device=dev, dtype=f32)
        L.check(L.lib().t2_hifigan_mpd_pack(wp, bp, L.ptr(packed), L.stream()))
        packed_bwd = None
        if backward_pack:
            packed_bwd = torch.empty(plan.packed_bwd_bytes // 4, device=dev, dtype=f32)
            L.check(L.lib().t2_hifigan_mpd_pack_backward(wp, L.ptr(packed_bwd), L.stream()))
        fmaps = [torch.empty(B, plan.C[i + 1], plan.H[i + 1], period, device=dev, dtype=f32) for i in range(n)]
        a = L.HifiganMpdFwdArgs(period, B, T, L.ptr(packed), L.ptr(audio), (C.c_void_p * n)(*[L.ptr(f) for f in fmaps]))
        L.check(L.lib().t2_hifigan_mpd_forward(C.byref(a), L.stream()))
    return fmaps, packed, packed_bwd


class _DiscriminatorPFunction(torch.autograd.Function):
    """The six feature maps of one period discriminator from the audio [B, 1, T] (real and generated items together) and the folded
    fp32 tensors (weight, bias per conv).  The weights are packed on every call: the parameters change between calls, and an optimizer
    that writes through raw pointers leaves no trace in a parameter's version.  The feature maps are the tape.  The backward takes
    whatever gradient autograd has for each map (none is a null pointer), launches the weight gradients only where a folded tensor
    asks for one and the audio's only where the audio does, and returns the parameters' as views into one arena."""

    @staticmethod
    def forward(ctx, period, audio, *tensors):
        audio = audio.detach().contiguous()
        fmaps, packed, packed_bwd = _mpd_launch(period, audio, tensors, True)
        ctx.period, ctx.packed, ctx.packed_bwd = period, packed, packed_bwd
        ctx.shapes = [t.shape for t in tensors]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(audio, *fmaps)
        return tuple(fmaps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g):
        audio, *fmaps = ctx.saved_tensors
        dev, f32 = audio.device, torch.float32
        B, _, T = audio.shape
        n = L.HIFIGAN_MPD_LAYERS
        plan = L.hifigan_mpd_plan(ctx.period, B, T)
        want_w, want_x = any(ctx.needs_input_grad[2:]), ctx.needs_input_grad[1]
        grads = [None] * len(ctx.shapes)
        if not (want_w or want_x) or all(x is None for x in g):
            return (None, None, *grads)
        with torch.cuda.device(dev):
            g = [None if x is None else x.to(f32).contiguous() for x in g]
            if g[n - 1] is None:
                g[n - 1] = torch.zeros_like(fmaps[n - 1])
            ws = torch.empty(plan.workspace_bytes // 4, device=dev, dtype=f32)
            arena = torch.empty(plan.grad_floats, device=dev, dtype=f32) if want_w else None
            d_audio = torch.empty_like(audio) if want_x else None
            a = L.HifiganMpdBwdArgs(ctx.period, B, T, L.ptr(ctx.packed), L.ptr(ctx.packed_bwd), L.ptr(audio),
                                    (C.c_void_p * n)(*[L.ptr(f) for f in fmaps]), (C.c_void_p * n)(*[L.ptr(x) for x in g]),
                                    L.ptr(ws), L.ptr(arena), L.ptr(d_audio))
            L.check(L.lib().t2_hifigan_mpd_backward(C.byref(a), L.stream()))
        if want_w:
            for i in range(n):
                ws_, bs_ = ctx.shapes[2 * i], ctx.shapes[2 * i + 1]
                wo, bo = plan.w_offsets[i], plan.b_offsets[i]
                # the weight's gradient is consumed by _weight_norm's backward; the bias's goes to the parameter, and a view kept as
                # .grad would pin the whole arena (33 MB per discriminator) for 4 KB: it is a copy of its own
                grads[2 * i], grads[2 * i + 1] = arena[wo:wo + ws_.numel()].view(ws_), arena[bo:bo + bs_.numel()].view(bs_).clone()
        return (None, d_audio, *grads)


class DiscriminatorP(nn.Module):
    """hifigan_model.py:127-160 with the reference's parameter names and shapes; ``forward`` runs csrc/vocoder_disc.hip."""

    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False):
        super().__init__()
        if use_spectral_norm:
            raise NotImplementedError("DiscriminatorP(use_spectral_norm=True): " + _MSD_NOT_BUILT)
        if kernel_size != 5 or stride != 3:
            raise NotImplementedError(f"DiscriminatorP(kernel_size={kernel_size}, stride={stride}): " + _MSD_NOT_BUILT)
        self.period = int(period)
        L.hifigan_mpd_plan(self.period, 1, self.period)  # refuses an unsupported period here, by name
        self.convs = nn.ModuleList([_WNConv2d(_MPD_WIDTHS[i], _MPD_WIDTHS[i + 1], 5) for i in range(5)])
        self.conv_post = _WNConv2d(_MPD_WIDTHS[5], 1, 3)

    def _maps(self, x):
        """The six feature maps for x [B, 1, T]: with a gradient wherever grad mode is on and x or a parameter asks for one."""
        who = "hifigan DiscriminatorP"
        if not x.is_cuda:
            raise RuntimeError(f"{who}: the audio must live on the GPU (the product path has no CPU fallback)")
        if x.dim() != 3 or x.shape[1] != 1:
            raise RuntimeError(f"{who}: expected audio of shape [B, 1, T], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"{who}: the audio must be float32, got {x.dtype}")
        layers = list(self.convs) + [self.conv_post]
        if layers[0].bias.device != x.device:
            raise RuntimeError(f"{who}: the audio is on {x.device}, the parameters on {layers[0].bias.device}")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            tensors = []
            for l in layers:
                tensors += [torch._weight_norm(l.weight_v, l.weight_g, 0), l.bias]
            return list(_DiscriminatorPFunction.apply(self.period, x, *tensors))
        with torch.no_grad():                            # only the forward runs and nothing is kept
            tensors = []
            for l in layers:
                tensors += [torch._weight_norm(l.weight_v, l.weight_g, 0), l.bias]
            return _mpd_launch(self.period, x.detach().contiguous(), tensors, False)[0]

    def forward(self, x):
        fmap = self._maps(x)
        return torch.flatten(fmap[-1], 1, -1), fmap


class MultiPeriodDiscriminator(nn.Module):
    """hifigan_model.py:163-187.  Real and generated audio run through each period discriminator as one batch of 2B items, so the
    weights are read once; an item's feature maps have the bits of the item run alone."""

    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorP(p) for p in (2, 3, 5, 7, 11)])

    def forward(self, y, y_hat):
        if y.shape != y_hat.shape:
            raise RuntimeError(f"hifigan MultiPeriodDiscriminator: y is {tuple(y.shape)}, y_hat {tuple(y_hat.shape)}")
        B = y.shape[0]
        both = torch.cat([y, y_hat], dim=0)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for d in self.discriminators:
            maps = d._maps(both)
            fmap_r, fmap_g = [m[:B] for m in maps], [m[B:] for m in maps]
            y_d_rs.append(torch.flatten(fmap_r[-1], 1, -1))
            y_d_gs.append(torch.flatten(fmap_g[-1], 1, -1))
            fmap_rs.append(fmap_r)
            fmap_gs.append(fmap_g)
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs


def feature_loss(fmap_r, fmap_g):
    """hifigan_model.py:250-256: twice the sum over every feature map of the mean absolute difference."""
    total = 0
    for maps_r, maps_g in zip(fmap_r, fmap_g):
        for r, g in zip(maps_r, maps_g):
            total = total + (r - g).abs().mean()
    return total * 2


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """hifigan_model.py:259-270: least squares, real scores towards 1 and generated towards 0; the per-discriminator terms as floats."""
    total, r_losses, g_losses = 0, [], []
    for real, fake in zip(disc_real_outputs, disc_generated_outputs):
        r_term, g_term = ((1 - real) ** 2).mean(), (fake ** 2).mean()
        total = total + (r_term + g_term)
        r_losses.append(r_term.item())
        g_losses.append(g_term.item())
    return total, r_losses, g_losses


def generator_loss(disc_outputs):
    """hifigan_model.py:273-281: least squares, generated scores towards 1; the per-discriminator terms stay tensors."""
    total, gen_losses = 0, []
    for fake in disc_outputs:
        term = ((1 - fake) ** 2).mean()
        gen_losses.append(term)
        total = total + term
    return total, gen_losses
