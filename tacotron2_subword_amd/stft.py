"""Mel front end used for real (non-synthetic) GTA extraction (reference: stft.py:42-105,
layers.py:42-80, audio_processing.py:78-93), and the synthesis side the vocoder's bias remover and Griffin-Lim need
(stft.py:107-141).

`STFT.transform` = reflect-pad by filter_length/2, frame with stride hop_length, multiply by the windowed Fourier
basis [2*(N/2+1), N] (the reference does this as a strided conv1d), magnitude + phase.  Here the frames x basis
product runs on the HIP GEMM (`ops.gemm`, fp32 MFMA: a 1024-tap basis is a plain [frames, 1024] x [1024, 1026]
product); on CPU tensors it falls back to torch.matmul only so that the formula can be compared with the reference's
own STFT on the GPU-less build box (tests/golden/make_golden_stft.py) — this module is not part of the model's hot path.

`STFT.inverse` runs csrc/stft.hip's synthesis kernel: the conv_transpose1d with the inverse basis as an overlap-add GEMM
(DESIGN.md "STFT synthesis"), magnitude * (cos, sin)(phase) formed in its loader, the window sum-square envelope, the
N/hop scale and the trim in its epilogue: one launch.  The module-level `analysis` / `synthesis` / `pack_tables` are the
kernels' entry points (bias_remover.py uses them; the tests drive them with bases of their own).  On CPU tensors
`inverse` is the torch formula, for the same comparison only.

`log_mel` is the whole mel front end in one launch of csrc/melspec.hip (DESIGN.md "Log-mel front end"): framing with
reflect padding as index arithmetic on each item's own length, the Fourier and the mel product on the fp32 matrix cores
with the magnitudes kept in LDS between them, clamp and log in the epilogue.  `TacotronSTFT.mel_spectrogram` goes through
it for CUDA tensors (layers.py:60-80), `utils.mel_spectrogram` with the HiFi-GAN convention's padding (utils.py:73-79);
`STFT.transform` itself is unchanged.

The mel filterbank restates librosa.filters.mel (Slaney mel scale, Slaney area normalisation), which the reference
calls as librosa_mel_fn(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax) (layers.py:48-49).  librosa is
not installed here, so the filterbank itself is "parity unpinned" (property tests only); the STFT magnitudes are pinned
by the reference's stft.py."""
import numpy as np
import torch
from scipy.signal import get_window

from .audio_processing import _pad_center, dynamic_range_compression, dynamic_range_decompression, window_sumsquare


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """[n_mels, 1 + n_fft//2] triangular filters, Slaney scale and normalisation (librosa.filters.mel defaults)."""
    fmax = float(sr) / 2 if fmax is None else fmax
    fftfreqs = np.linspace(0, float(sr) / 2, int(1 + n_fft // 2), endpoint=True)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, int(1 + n_fft // 2)))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return (weights * enorm[:, np.newaxis]).astype(np.float32)


def _check_planes(who, a, b, bins):
    if a.dim() != 3 or a.shape != b.shape or a.shape[1] != bins:
        raise RuntimeError(f"{who}: expected two tensors of one shape [B, {bins}, frames], got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError(f"{who}: the inputs must be float32, got {a.dtype} and {b.dtype}")
    if a.device != b.device:
        raise RuntimeError(f"{who}: the inputs are on {a.device} and {b.device}")
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        raise RuntimeError(f"{who} is inference only: an input requires grad and grad mode is on; call it under torch.no_grad() "
                           "or detach the inputs")


def pack_tables(forward_basis, inverse_basis, window_sq, filter_length, hop_length):
    """The tables of csrc/stft.hip in the order its lanes read them (t2_stft_pack).  forward_basis, inverse_basis:
    [2*(N/2+1), N] fp32 on the GPU; window_sq: the squared, centre-padded window [N] in fp64, or None (no window)."""
    from . import _lib as L
    plan = L.stft_plan(filter_length, hop_length)
    rows = 2 * plan.bins
    for name, t in (("forward_basis", forward_basis), ("inverse_basis", inverse_basis)):
        if tuple(t.shape) != (rows, filter_length) or t.dtype != torch.float32:
            raise RuntimeError(f"stft pack_tables: {name} must be float32 [{rows}, {filter_length}], got {t.dtype} {tuple(t.shape)}")
    if window_sq is not None and (tuple(window_sq.shape) != (filter_length,) or window_sq.dtype != torch.float64):
        raise RuntimeError(f"stft pack_tables: window_sq must be float64 [{filter_length}], got {window_sq.dtype} {tuple(window_sq.shape)}")
    dev = forward_basis.device
    with torch.cuda.device(dev):
        packed = torch.empty(plan.packed_bytes // 4, device=dev, dtype=torch.float32)
        L.check(L.lib().t2_stft_pack(filter_length, hop_length, L.ptr(forward_basis.contiguous()), L.ptr(inverse_basis.contiguous()),
                                     L.ptr(None if window_sq is None else window_sq.contiguous()), L.ptr(packed), L.stream()))
    return packed


class _AnalysisFn(torch.autograd.Function):
    """`analysis` for want within (re, im) with a backward: csrc/stft.hip's overlap-add GEMM with the forward basis and the
    fold of the reflect padding (t2_stft_analysis_backward).  Saves the lengths only: the gradient does not depend on x."""

    @staticmethod
    def forward(ctx, x, launch, grad_packed, lengths, cfg):
        ctx.cfg = cfg
        ctx.save_for_backward(grad_packed, lengths)
        return launch()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        from . import _lib as L
        N, hop, want, B, n, fwd_floats = ctx.cfg
        packed, lengths = ctx.saved_tensors
        dev = packed.device
        g = {k: (None if v is None else v.contiguous()) for k, v in zip(want, grads)}
        with torch.cuda.device(dev):
            dx = torch.empty(B, n, device=dev, dtype=torch.float32)
            if g.get("re") is None and g.get("im") is None:
                return (dx.zero_(),) + (None,) * 4
            dxpad = torch.empty(B * (n + N), device=dev, dtype=torch.float32)
            a = L.StftAnalysisBackwardArgs(B, N, hop, n, L.ptr(g.get("re")), L.ptr(g.get("im")), packed.data_ptr() + 4 * fwd_floats,
                                           L.ptr(lengths), L.ptr(dxpad), L.ptr(dx))
            L.check(L.lib().t2_stft_analysis_backward(a, L.stream()))
        return (dx,) + (None,) * 4


def analysis(x, packed, filter_length, hop_length, want=("re", "im"), lengths=None, differentiable=False, grad_packed=None):
    """x [B, n] fp32 on the GPU -> the tensors named in `want` (of "re", "im", "mag", "phase"), [B, N/2+1, 1 + n//hop]
    each, from one launch of the analysis kernel; the reflect padding is the kernel's index arithmetic.
    lengths: per-item sample counts in the convention of `log_mel` (Python ints, checked here, or an int32 device tensor [B],
    clamped to [0, n] by the kernel, no host sync).  Item b is then x[b, :lengths[b]] alone, bit for bit: its own reflection,
    1 + lengths[b]//hop frames, zeros behind them; what the row holds behind its length is never read.  The int32 device
    tensor of those frame counts is returned after the tensors of `want`.  An item of <= N/2 samples raises in torch's
    reflect-pad words when given as a Python int; in a device tensor it has no frames: all zero, count 0.
    differentiable=True (opt-in): an x that requires grad under grad mode gives re / im with a grad_fn (once differentiable,
    no gradient for the bases); grad_packed is then `pack_tables` of (forward_basis, forward_basis, None), whose synthesis-order
    part is the backward's table (STFT.grad_tables()).  "mag" and "phase" have no backward."""
    from . import _lib as L
    if x.dim() != 2 or x.dtype != torch.float32:
        raise RuntimeError(f"stft analysis: expected a float32 signal [B, n], got {x.dtype} {tuple(x.shape)}")
    track = torch.is_grad_enabled() and x.requires_grad
    if track and not differentiable:
        raise RuntimeError("stft analysis is inference only: the input requires grad and grad mode is on")
    if differentiable:
        for k in want:
            if k not in ("re", "im"):
                raise RuntimeError(f'stft analysis: differentiable=True has no backward for "{k}": only "re" and "im" are differentiable')
        if grad_packed is None:
            raise RuntimeError("stft analysis: differentiable=True needs grad_packed (STFT.grad_tables())")
    B, n = x.shape
    half = filter_length // 2
    if n <= half:        # torch's own words for F.pad(..., mode="reflect")
        raise RuntimeError(f"Padding size should be less than the corresponding input dimension, but got: padding ({half}, {half}) "
                           f"at dimension 1 of input {list(x.shape)}")
    plan = L.stft_plan(filter_length, hop_length, 1 + n // hop_length)
    x_in, x = x, x.detach().contiguous()
    if lengths is not None:
        def too_short(i, v):
            return RuntimeError(f"Padding size should be less than the corresponding input dimension, but got: padding ({half}, {half}) "
                                f"at dimension 1 of item {i} of {v} samples")
        lengths = L.lengths_arg("stft analysis", lengths, B, n, x.device, lo=half + 1, too_short=too_short)
    box = {}

    def launch():
        with torch.cuda.device(x.device):
            out = {k: torch.empty(B, plan.bins, 1 + n // hop_length, device=x.device, dtype=torch.float32) for k in want}
            planes = [L.ptr(out.get(k)) for k in ("re", "im", "mag", "phase")]
            if lengths is None:
                a = L.StftAnalysisArgs(B, filter_length, hop_length, n, L.ptr(x), L.ptr(packed), *planes)
                L.check(L.lib().t2_stft_analysis(a, L.stream()))
            else:
                box["frame_lengths"] = torch.empty(B, device=x.device, dtype=torch.int32)
                a = L.StftAnalysisRaggedArgs(B, filter_length, hop_length, n, L.ptr(x), L.ptr(packed), *planes, L.ptr(lengths), L.ptr(box["frame_lengths"]))
                L.check(L.lib().t2_stft_analysis_ragged(a, L.stream()))
        return tuple(out[k] for k in want)

    res = _AnalysisFn.apply(x_in, launch, grad_packed, lengths, (filter_length, hop_length, tuple(want), B, n, plan.fwd_floats)) if track else launch()
    return tuple(res) if lengths is None else tuple(res) + (box["frame_lengths"],)


def synthesis(a, b, packed, filter_length, hop_length, mode=0, bias=None, strength=0.0, windowed=True, lengths=None):
    """Two planes [B, N/2+1, nf] fp32 on the GPU -> audio [B, 1, hop*(nf-1)] from one launch of the synthesis kernel.
    mode 0 (polar): a = magnitude, b = phase.  mode 1 (denoise): a = re, b = im, bias [N/2+1] and strength: the bias
    remover's clamp(|z| - strength*bias, 0) applied as a gain.  windowed=False leaves out the envelope division and the
    N/hop scale (STFT(window=None)): the output is then the trimmed overlap-add sum itself.
    lengths: per-item frame counts in the convention of `log_mel` (Python ints in [1, nf], checked here, or an int32 device
    tensor [B], clamped to [0, nf] by the kernel, no host sync).  Item b is then its first lengths[b] frames alone, bit for
    bit; the planes behind them are never read, the audio is zero from hop*(lengths[b]-1) on, and the result is
    (audio, sample_lengths) with those counts as an int32 device tensor.  A count below 1 in a device tensor gives an
    all-zero row of length 0."""
    from . import _lib as L
    plan = L.stft_plan(filter_length, hop_length, max(int(a.shape[-1]), 1) if a.dim() == 3 else 1)
    _check_planes("stft synthesis", a, b, plan.bins)
    B, _, nf = a.shape
    if nf < 1:
        raise RuntimeError("stft synthesis: no frames")
    if mode == L.STFT_DENOISE and (bias is None or bias.numel() != plan.bins or bias.dtype != torch.float32):
        raise RuntimeError(f"stft synthesis: the denoise mode needs a float32 bias spectrum of {plan.bins} bins")
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if lengths is not None:
        def no_frames(i, v):
            return RuntimeError(f"stft synthesis: no frames: lengths[{i}]={v}")
        lengths = L.lengths_arg("stft synthesis", lengths, B, nf, a.device, lo=1, too_short=no_frames)
    with torch.cuda.device(a.device):
        y = torch.empty(B, 1, plan.out_len, device=a.device, dtype=torch.float32)
        common = (B, filter_length, hop_length, nf, mode, int(bool(windowed)), L.ptr(a), L.ptr(b),
                  L.ptr(None if bias is None else bias.detach().reshape(-1).contiguous()), float(strength), L.ptr(packed), L.ptr(y))
        if lengths is None:
            L.check(L.lib().t2_stft_synthesis(L.StftSynthesisArgs(*common), L.stream()))
            return y
        sample_lengths = torch.empty(B, device=a.device, dtype=torch.int32)
        L.check(L.lib().t2_stft_synthesis_ragged(L.StftSynthesisRaggedArgs(*common, L.ptr(lengths), L.ptr(sample_lengths)), L.stream()))
    return y, sample_lengths


def pack_mel_tables(forward_basis, mel_basis, filter_length):
    """The tables of csrc/melspec.hip (t2_melspec_pack): forward_basis [2*(N/2+1), N] and mel_basis [n_mels, N/2+1], fp32
    on the GPU."""
    from . import _lib as L
    bins = filter_length // 2 + 1
    if tuple(forward_basis.shape) != (2 * bins, filter_length) or forward_basis.dtype != torch.float32:
        raise RuntimeError(f"log_mel: forward_basis must be float32 [{2 * bins}, {filter_length}], got {forward_basis.dtype} {tuple(forward_basis.shape)}")
    if mel_basis.dim() != 2 or mel_basis.shape[1] != bins or mel_basis.dtype != torch.float32:
        raise RuntimeError(f"log_mel: mel_basis must be float32 [n_mels, {bins}], got {mel_basis.dtype} {tuple(mel_basis.shape)}")
    if mel_basis.device != forward_basis.device:
        raise RuntimeError(f"log_mel: mel_basis is on {mel_basis.device}, the STFT module on {forward_basis.device}")
    n_mels = int(mel_basis.shape[0])
    plan = L.melspec_plan(filter_length, filter_length, filter_length // 2, n_mels, filter_length)
    dev = forward_basis.device
    with torch.cuda.device(dev):
        packed = torch.empty(plan.packed_bytes // 4, device=dev, dtype=torch.float32)
        L.check(L.lib().t2_melspec_pack(filter_length, n_mels, L.ptr(forward_basis.detach().contiguous()), L.ptr(mel_basis.detach().contiguous()),
                                        L.ptr(packed), L.stream()))
    return packed


def pack_mel_grad_tables(forward_basis, mel_basis, filter_length, hop_length):
    """The backward's tables (t2_melspec_grad_pack): the mel basis in the transposed product's order, then the forward basis in
    the synthesis kernel's order.  Arguments as `pack_mel_tables`."""
    from . import _lib as L
    n_mels = int(mel_basis.shape[0])
    plan = L.melspec_grad_plan(filter_length, hop_length, filter_length // 2, n_mels, filter_length)
    dev = forward_basis.device
    with torch.cuda.device(dev):
        packed = torch.empty(plan.packed_bytes // 4, device=dev, dtype=torch.float32)
        L.check(L.lib().t2_melspec_grad_pack(filter_length, hop_length, n_mels, L.ptr(forward_basis.detach().contiguous()),
                                             L.ptr(mel_basis.detach().contiguous()), L.ptr(packed), L.stream()))
    return packed


class _LogMelFn(torch.autograd.Function):
    """`log_mel` with a backward (csrc/melspec.hip melspec_grad_kernel, csrc/stft.hip stft_analysis_backward).  Keeps x, the
    lengths and the mel sum s; re and im are recomputed.  Once differentiable; no gradient for the bases."""

    @staticmethod
    def forward(ctx, x, launch, cfg, box):
        xc, lengths, mel, frame_lengths, s = launch()
        box["frame_lengths"] = frame_lengths
        ctx.cfg = cfg
        ctx.save_for_backward(xc, lengths, s)
        return mel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from . import _lib as L
        stft_module, mel_basis, pad, mag_eps, clip_val, time_major = ctx.cfg
        x, lengths, s = ctx.saved_tensors
        N, hop = stft_module.filter_length, stft_module.hop_length
        B, n = x.shape
        n_mels = int(mel_basis.shape[0])
        plan = L.melspec_grad_plan(N, hop, pad, n_mels, n, B)
        dev = x.device
        with torch.cuda.device(dev):
            g = g.contiguous()
            ws = torch.empty(plan.workspace_floats, device=dev, dtype=torch.float32)
            dx = torch.empty_like(x)
            a = L.MelspecBackwardArgs(B, N, hop, pad, n_mels, n, L.ptr(x), L.ptr(lengths), L.ptr(stft_module.mel_tables(mel_basis)),
                                      L.ptr(stft_module.mel_grad_tables(mel_basis)), L.ptr(s), L.ptr(g), L.ptr(ws), ws.numel(), L.ptr(dx),
                                      float(mag_eps), float(clip_val), int(bool(time_major)))
            L.check(L.lib().t2_melspec_backward(a, L.stream()))
        return dx, None, None, None


def log_mel(x, stft_module, mel_basis, lengths=None, pad=None, mag_eps=0.0, clip_val=1e-5, C=1, time_major=False, pad_value=0.0,
            *, force_splits=0, return_power=False, out=None, scratch=None, differentiable=False):
    """x [B, n] fp32 on the GPU -> (mel, frame_lengths) from one launch of csrc/melspec.hip:
        mel[b, m, f] = log(max(clip_val, sum_bin mel_basis[m, bin] * sqrt(re^2 + im^2 + mag_eps)) * C)
    over the frames of x[b, :lengths[b]] reflect-padded by `pad` per side.  pad=None is filter_length/2 (TacotronSTFT,
    layers.py:76-79); pad=(N - hop)/2 with mag_eps=1e-9 is utils.mel_spectrogram's torch.stft(center=False) (utils.py:73-79).
    mel is [B, n_mels, nf_max], or [B, nf_max, n_mels] with time_major (what SoftDTW takes); nf_max follows from n.  Frames
    past an item's own count hold pad_value.  lengths: None, an int32 device tensor [B] (clamped to [0, n] by the kernel, no
    host sync; an item of <= pad samples has no frames), or Python ints, which are checked here: a too-short item raises in
    torch's reflect-pad words.  frame_lengths is an int32 device tensor [B], or None when lengths is.
    The keyword-only arguments are for the tests: force_splits (the launch shape; the bits do not depend on it), return_power
    (the mel sum over re^2 + im^2 + mag_eps, no clamp and no log), and caller-owned out / scratch buffers.
    differentiable=True (opt-in): an x that requires grad under grad mode gives a mel with a grad_fn, the same bits as
    without; its backward is HIP as well, once differentiable, with no gradient for the bases and no host
    synchronisation.  Where the magnitude is exactly 0 the gradient is 0, not torch's NaN; frames at the clip contribute 0.
    It needs hop_length dividing filter_length with at most 64 overlaps, and refuses return_power, out= and scratch=."""
    from . import _lib as L
    N, hop = stft_module.filter_length, stft_module.hop_length
    pad = N // 2 if pad is None else int(pad)
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise RuntimeError(f"log_mel: expected a float32 signal [B, n], got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    if not x.is_cuda:
        raise RuntimeError("log_mel: the signal must live on the GPU (there is no CPU path; TacotronSTFT.mel_spectrogram keeps the torch formula for CPU tensors)")
    track = torch.is_grad_enabled() and x.requires_grad
    if track and not differentiable:
        raise RuntimeError("log_mel is inference only: the input requires grad and grad mode is on; call it under torch.no_grad() or detach the input")
    if differentiable and (return_power or out is not None or scratch is not None):
        raise RuntimeError("log_mel: differentiable=True does not go with return_power, out= or scratch=")
    if stft_module.forward_basis.device != x.device:
        raise RuntimeError(f"log_mel: the input is on {x.device}, the STFT module on {stft_module.forward_basis.device}")
    B, n = x.shape
    n_mels = int(mel_basis.shape[0])

    def too_short(what, length):
        return RuntimeError(f"Padding size should be less than the corresponding input dimension, but got: padding ({pad}, {pad}) "
                            f"at dimension 1 of {what} of {length} samples")

    if n <= pad:
        raise too_short(f"input {list(x.shape)}", n)
    plan = L.melspec_plan(N, hop, pad, n_mels, n, B)
    if track:
        L.melspec_grad_plan(N, hop, pad, n_mels, n, B)         # what the backward refuses is refused here, by name
    dev = x.device
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        lengths = [int(v) for v in lengths]
        if len(lengths) != B:
            raise RuntimeError(f"log_mel: {len(lengths)} lengths for a batch of {B}")
        for i, v in enumerate(lengths):
            if v > n:
                raise RuntimeError(f"log_mel: lengths[{i}]={v} exceeds the {n} samples of a row")
            if v <= pad:
                raise too_short(f"item {i}", v)
            if v + 2 * pad < N:
                raise RuntimeError(f"log_mel: lengths[{i}]={v} with pad={pad} per side does not fill one frame of filter_length={N}")
        lengths = torch.tensor(lengths, dtype=torch.int32).to(dev)
    if lengths is not None:
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or lengths.device != dev:
            raise RuntimeError(f"log_mel: lengths must be int32 [{B}] on {dev}, got {lengths.dtype} {tuple(lengths.shape)} on {lengths.device}")
        lengths = lengths.contiguous()
    splits = int(force_splits) if force_splits else plan.splits
    shape = (B, plan.nf_max, n_mels) if time_major else (B, n_mels, plan.nf_max)
    xc = x.detach().contiguous()

    def launch(out=out, scratch=scratch):
        return _log_mel_launch(xc, stft_module, mel_basis, lengths, plan, shape, splits, out, scratch, track,
                               (B, N, hop, pad, n_mels, n, mag_eps, clip_val, C, pad_value, time_major, return_power, force_splits))

    if track:
        box = {}
        mel = _LogMelFn.apply(x, launch, (stft_module, mel_basis, pad, mag_eps, clip_val, time_major), box)
        return mel, box["frame_lengths"]
    _, _, out, frame_lengths, _ = launch()
    return out, frame_lengths


def _log_mel_launch(x, stft_module, mel_basis, lengths, plan, shape, splits, out, scratch, keep_sum, cfg):
    """The launch of `log_mel`: -> (x, lengths, out, frame_lengths, mel_sum); mel_sum [B, nf_max, n_mels] only with keep_sum."""
    from . import _lib as L
    B, N, hop, pad, n_mels, n, mag_eps, clip_val, C, pad_value, time_major, return_power, force_splits = cfg
    dev = x.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, device=dev, dtype=torch.float32)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev:
            raise RuntimeError(f"log_mel: out must be float32 {shape} on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        if splits > 1 and scratch is None:
            scratch = torch.empty(plan.split_scratch_floats, device=dev, dtype=torch.float32)
        if scratch is not None and (scratch.dtype != torch.float32 or scratch.device != dev):
            raise RuntimeError(f"log_mel: scratch must be float32 on {dev}, got {scratch.dtype} on {scratch.device}")
        frame_lengths = None if lengths is None else torch.empty(B, device=dev, dtype=torch.int32)
        mel_sum = torch.empty(B, plan.nf_max, n_mels, device=dev, dtype=torch.float32) if keep_sum else None
        a = L.MelspecArgs(B, N, hop, pad, n_mels, n, L.ptr(x), L.ptr(lengths), L.ptr(stft_module.mel_tables(mel_basis)), L.ptr(out),
                          L.ptr(scratch), 0 if scratch is None else scratch.numel(), L.ptr(frame_lengths),
                          float(mag_eps), float(clip_val), float(C), float(pad_value), int(bool(time_major)), int(bool(return_power)), int(force_splits),
                          L.ptr(mel_sum))
        L.check(L.lib().t2_melspec(a, L.stream()))
    return x, lengths, out, frame_lengths, mel_sum


class STFT(torch.nn.Module):
    def __init__(self, filter_length=800, hop_length=200, win_length=800, window="hann"):
        super().__init__()
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        scale = filter_length / hop_length
        fourier_basis = np.fft.fft(np.eye(filter_length))
        cutoff = int(filter_length / 2 + 1)
        fourier_basis = np.vstack([np.real(fourier_basis[:cutoff, :]), np.imag(fourier_basis[:cutoff, :])])
        forward_basis = torch.FloatTensor(fourier_basis[:, None, :])
        inverse_basis = torch.FloatTensor(np.linalg.pinv(scale * fourier_basis).T[:, None, :])
        if window is not None:
            assert filter_length >= win_length
            fft_window = torch.from_numpy(_pad_center(get_window(window, win_length, fftbins=True), filter_length)).float()
            forward_basis *= fft_window
            inverse_basis *= fft_window
        self.register_buffer("forward_basis", forward_basis.float())       # [2*cutoff, 1, N], the reference's buffer name / shape
        self.register_buffer("inverse_basis", inverse_basis.float())       # [2*cutoff, 1, N], likewise
        self._packed = None
        self._packed_key = None
        self._mel_packed = None
        self._mel_basis = None
        self._mel_key = None
        self._mel_grad_packed = None
        self._mel_grad_basis = None
        self._mel_grad_key = None
        self._grad_packed = None
        self._grad_key = None

    def _apply(self, fn, *args, **kwargs):                                  # .to() / .cuda(): the packed tables follow the buffers
        out = super()._apply(fn, *args, **kwargs)
        self._packed = None
        self._mel_packed = None
        self._mel_grad_packed = None
        self._grad_packed = None
        return out

    def _key(self):
        return tuple((t.data_ptr(), t._version) for t in (self.forward_basis, self.inverse_basis))

    def window_sq(self):
        """The squared window, centre-padded to filter_length, fp64: what window_sumsquare adds per frame.  None without a window."""
        if self.window is None:
            return None
        return _pad_center(get_window(self.window, self.win_length, fftbins=True) ** 2, self.filter_length)

    def tables(self):
        """The kernels' packed tables, built on first use and again after .to() / .cuda() / load_state_dict."""
        if not self.forward_basis.is_cuda:
            raise RuntimeError("STFT: the buffers must live on the GPU for the HIP kernels (module.cuda())")
        if self._packed is None or self._packed_key != self._key():
            wsq = self.window_sq()
            dev = self.forward_basis.device
            self._packed = pack_tables(self.forward_basis[:, 0, :], self.inverse_basis[:, 0, :],
                                       None if wsq is None else torch.from_numpy(wsq).to(dev), self.filter_length, self.hop_length)
            self._packed_key = self._key()
        return self._packed

    def mel_tables(self, mel_basis):
        """The log-mel kernel's packed tables for this module's forward basis and `mel_basis` [n_mels, N/2+1], built on first
        use and again after .to() / .cuda() / load_state_dict of either (the last mel basis is the one kept)."""
        if not self.forward_basis.is_cuda:
            raise RuntimeError("STFT: the buffers must live on the GPU for the HIP kernels (module.cuda())")
        # the mel basis is the caller's: its address alone could be that of an earlier, freed tensor, so the key holds the tensor
        key = (self.forward_basis.data_ptr(), self.forward_basis._version, mel_basis._version)
        if self._mel_packed is None or self._mel_basis is not mel_basis or self._mel_key != key:
            self._mel_packed = pack_mel_tables(self.forward_basis[:, 0, :], mel_basis, self.filter_length)
            self._mel_basis, self._mel_key = mel_basis, key
        return self._mel_packed

    def mel_grad_tables(self, mel_basis):
        """The log-mel backward's packed tables, kept like `mel_tables`."""
        if not self.forward_basis.is_cuda:
            raise RuntimeError("STFT: the buffers must live on the GPU for the HIP kernels (module.cuda())")
        key = (self.forward_basis.data_ptr(), self.forward_basis._version, mel_basis._version)
        if self._mel_grad_packed is None or self._mel_grad_basis is not mel_basis or self._mel_grad_key != key:
            self._mel_grad_packed = pack_mel_grad_tables(self.forward_basis[:, 0, :], mel_basis, self.filter_length, self.hop_length)
            self._mel_grad_basis, self._mel_grad_key = mel_basis, key
        return self._mel_grad_packed

    def grad_tables(self):
        """What `analysis(..., differentiable=True)` takes as grad_packed: `pack_tables` with the forward basis in the inverse
        basis' place, so that its synthesis-order part drives the backward's overlap-add."""
        if not self.forward_basis.is_cuda:
            raise RuntimeError("STFT: the buffers must live on the GPU for the HIP kernels (module.cuda())")
        key = (self.forward_basis.data_ptr(), self.forward_basis._version)
        if self._grad_packed is None or self._grad_key != key:
            fwd = self.forward_basis[:, 0, :]
            self._grad_packed = pack_tables(fwd, fwd, None, self.filter_length, self.hop_length)
            self._grad_key = key
        return self._grad_packed

    def transform(self, input_data):
        B, n = input_data.shape
        half = int(self.filter_length / 2)
        x = torch.nn.functional.pad(input_data.view(B, 1, 1, n), (half, half, 0, 0), mode="reflect").view(B, -1)
        frames = x.unfold(1, self.filter_length, self.hop_length)           # [B, n_frames, N]
        nf = frames.shape[1]
        basis = self.forward_basis[:, 0, :]                                  # [2*cutoff, N]
        flat = frames.reshape(B * nf, self.filter_length).contiguous()
        if flat.is_cuda:
            from . import ops
            ft = ops.gemm(flat, basis.contiguous(), trans_b=True)            # HIP GEMM: [B*nf, 2*cutoff]
        else:
            ft = flat @ basis.t()
        ft = ft.view(B, nf, -1).transpose(1, 2)                              # [B, 2*cutoff, nf] like the conv1d output
        cutoff = int(self.filter_length / 2 + 1)
        real_part, imag_part = ft[:, :cutoff, :], ft[:, cutoff:, :]
        return torch.sqrt(real_part ** 2 + imag_part ** 2), torch.atan2(imag_part, real_part)

    def inverse(self, magnitude, phase):
        """magnitude, phase [B, N/2+1, frames] -> audio [B, 1, hop*(frames-1)] (stft.py:107-136)."""
        cutoff = int(self.filter_length / 2 + 1)
        _check_planes("STFT.inverse", magnitude, phase, cutoff)
        if not magnitude.is_cuda:
            return self._inverse_torch(magnitude, phase)
        if self.forward_basis.device != magnitude.device:
            raise RuntimeError(f"STFT.inverse: the input is on {magnitude.device}, the module on {self.forward_basis.device}")
        return synthesis(magnitude, phase, self.tables(), self.filter_length, self.hop_length, windowed=self.window is not None)

    def _inverse_torch(self, magnitude, phase):
        """The reference's formula in torch ops, for CPU tensors: comparison with the reference on a box without a GPU."""
        half = int(self.filter_length / 2)
        x = torch.cat([magnitude * torch.cos(phase), magnitude * torch.sin(phase)], dim=1)
        y = torch.nn.functional.conv_transpose1d(x, self.inverse_basis, stride=self.hop_length, padding=0)
        if self.window is not None:
            env = window_sumsquare(self.window, magnitude.size(-1), hop_length=self.hop_length, win_length=self.win_length,
                                   n_fft=self.filter_length, dtype=np.float32)
            nonzero = torch.from_numpy(np.where(env > np.finfo(env.dtype).tiny)[0])
            env = torch.from_numpy(env).to(y.device)
            y[:, :, nonzero] /= env[nonzero]
            y *= float(self.filter_length) / self.hop_length
        return y[:, :, half:][:, :, :-half]

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)


class TacotronSTFT(torch.nn.Module):
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=22050,
                 mel_fmin=0.0, mel_fmax=8000.0):
        super().__init__()
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.stft_fn = STFT(filter_length, hop_length, win_length)
        self.register_buffer("mel_basis", torch.from_numpy(mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)).float())
        self._differentiable = False

    def differentiable(self, flag=True):
        """Opt in to a backward from the mel to the waveform on the GPU (`log_mel(..., differentiable=True)`); returns self,
        like WaveGlow.trainable()."""
        self._differentiable = bool(flag)
        return self

    def spectral_normalize(self, magnitudes):
        return dynamic_range_compression(magnitudes)

    def spectral_de_normalize(self, magnitudes):
        return dynamic_range_decompression(magnitudes)

    def mel_spectrogram(self, y, lengths=None, time_major=False):
        """y: [B, T] in [-1, 1] -> log-mel [B, n_mel_channels, frames] (layers.py:60-80).  CUDA tensors go through the log-mel
        kernel (`log_mel`: one launch, no frame matrix, no phase); CPU tensors keep the torch formula, for comparison.
        lengths (an addition): per-item sample counts, see `log_mel`; the result is then (mel, frame_lengths) and frames
        past an item's own hold 0, what the collate function pads mels with.  time_major gives [B, frames, n_mel_channels]."""
        assert torch.min(y.data) >= -1
        assert torch.max(y.data) <= 1
        if y.is_cuda:
            mel, frame_lengths = log_mel(y, self.stft_fn, self.mel_basis, lengths=lengths, time_major=time_major, differentiable=self._differentiable)
            return mel if lengths is None else (mel, frame_lengths)
        if lengths is not None:
            raise RuntimeError("TacotronSTFT.mel_spectrogram: per-item lengths need the HIP kernel (CUDA tensors)")
        magnitudes, _ = self.stft_fn.transform(y)
        mel = self.spectral_normalize(torch.matmul(self.mel_basis, magnitudes.data))
        return mel.transpose(1, 2).contiguous() if time_major else mel
