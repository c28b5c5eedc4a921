"""remove_silence.py of the reference (:7-36; the same function and loop are best_checkpoint.py:319-333 and :495-520): the
pydub trim of leading and trailing silence, for 16-bit mono audio that stays on the GPU.

The reference reads a wav file into a pydub.AudioSegment, finds the first 10 ms chunk whose dBFS is not below -50 from the
front and from the back, and writes sound[start : len(sound) - end] to another file.  Here the audio is a padded batch
[B, n] with per-item lengths, as the ragged vocoder and bias remover leave it, and the result is a padded batch with new
lengths, ready for TacotronSTFT.mel_spectrogram(y, lengths=...).  The arithmetic is pydub's, restated in include/t2amd.h
and decided in integers by csrc/silence.hip: every item has the bits the reference's trim gives for it alone.  Nothing
here synchronises with the host except where a Python value is asked for (a 1-D detect_leading_silence, silence_stats)."""
import ctypes as C

import torch

from . import _lib as L

_INT16_SCALE = 1.0 / 32768.0      # load_wav_to_torch(...) / max_wav_value, bit for bit


def _batch(who, sound):
    if not isinstance(sound, torch.Tensor) or sound.dim() not in (1, 2) or sound.dtype not in (torch.int16, torch.float32):
        raise RuntimeError(f"{who}: expected an int16 tensor, or a float32 one in int16 units, of shape [n] or [B, n], got "
                           f"{getattr(sound, 'dtype', type(sound))} {tuple(getattr(sound, 'shape', ()))}")
    if not sound.is_cuda:
        raise RuntimeError(f"{who}: the trim is a HIP kernel and needs a GPU: the audio must be a CUDA tensor (there is no CPU path)")
    x = sound.detach()
    x = x.unsqueeze(0) if x.dim() == 1 else x
    if x.shape[0] < 1:
        raise RuntimeError(f"{who}: an empty batch")
    return x.contiguous()


def _run(who, x, lengths, sample_rate, silence_threshold, chunk_size, out_dtype, scale, leading_only):
    B, n = x.shape
    dev = x.device
    plan = L.silence_plan(int(sample_rate), int(chunk_size), float(silence_threshold), n, B)
    lens = None if lengths is None else L.lengths_arg(who, lengths, B, n, dev)
    start = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(plan.scratch_bytes // 4, dtype=torch.int32, device=dev)
    out = new = end = None
    if not leading_only:
        out = torch.empty(B, plan.out_width, dtype=out_dtype, device=dev)
        new = torch.empty(B, dtype=torch.int32, device=dev)
        end = torch.empty(B, dtype=torch.int32, device=dev)
    args = L.SilenceArgs(B, n, int(sample_rate), int(chunk_size), float(silence_threshold), L.ptr(x), int(x.dtype == torch.float32),
                         L.ptr(lens), L.ptr(out), int(out_dtype == torch.float32), float(scale), L.ptr(new), L.ptr(start), L.ptr(end),
                         L.ptr(scratch), plan.scratch_bytes, int(leading_only))
    with torch.cuda.device(dev):
        L.check(L.lib().t2_silence_trim(C.byref(args), L.stream()))
    return out, new, start, end


def detect_leading_silence(sound, silence_threshold=-50.0, chunk_size=10, *, lengths=None, sample_rate=22050):
    """remove_silence.py:7-20.  sound: int16 (or float32 in int16 units) on the GPU.  A 1-D tensor gives the reference's return
    value, the leading silence in ms as a Python int, or None (this reads the result back).  [B, n] gives an int32 device
    tensor [B] with -1 for None and reads nothing back.  The trailing silence is detect_leading_silence(sound.flip(-1))."""
    who = "remove_silence.detect_leading_silence"
    x = _batch(who, sound)
    _, _, start, _ = _run(who, x, lengths, sample_rate, silence_threshold, chunk_size, torch.int16, 1.0, True)
    if sound.dim() == 1:
        v = int(start.item())
        return None if v < 0 else v
    return start


def trim_silence(audio, lengths=None, sample_rate=22050, silence_threshold=-50.0, chunk_size=10, out_dtype=torch.int16, scale=None):
    """remove_silence.py:25-36 for a padded batch.  audio [B, n] (or [n]) int16, or float32 in int16 units (clamped to the int16
    range and truncated toward zero, as best_checkpoint.py:216-224 does with astype('int16')); lengths: None, a list of ints
    or an int32 device tensor [B].
    Returns (trimmed, new_lengths, start_ms, end_ms): trimmed [B, n + int(0.5 * sample_rate / 1000) + 1] in out_dtype, each
    row holding sound[start : len(sound) - end] at its front and zeros behind new_lengths[b]; the three vectors int32 [B] on
    the device.  An entirely silent item (the reference skips it) has length 0 and start_ms = end_ms = -1.
    out_dtype=torch.float32 gives int16 * scale, scale = 1 / 32768 by default: load_wav_to_torch(...) / max_wav_value bit for
    bit, what mel_spectrogram takes."""
    who = "remove_silence.trim_silence"
    x = _batch(who, audio)
    if out_dtype not in (torch.int16, torch.float32):
        raise RuntimeError(f"{who}: out_dtype must be torch.int16 or torch.float32, got {out_dtype}")
    if scale is not None and out_dtype != torch.float32:
        raise RuntimeError(f"{who}: scale={scale} applies to out_dtype=torch.float32 only")
    out, new, start, end = _run(who, x, lengths, sample_rate, silence_threshold, chunk_size, out_dtype,
                                _INT16_SCALE if scale is None else scale, False)
    if audio.dim() == 1:
        return out[0], new[0], start[0], end[0]
    return out, new, start, end


def silence_stats(start_ms, limit_silence=3000, end_ms=None):
    """The counters the reference keeps per checkpoint (best_checkpoint.py:506-520) from trim_silence's start_ms:
    (start_silence, limit_silence, dropped) = the summed leading silence in ms of the items whose start was found, how many of
    them had limit_silence ms or more of it, and how many items were entirely silent.  With end_ms, an item whose start was
    found but whose end was not (the reference's loop raises on it and writes no file, after it has counted the start) is
    counted as dropped too.  Reads the three numbers back."""
    s = start_ms.reshape(-1).to(torch.int64)
    kept = s >= 0
    lost = ~kept if end_ms is None else ~kept | (end_ms.reshape(-1) < 0)
    vals = torch.stack([(s * kept).sum(), (kept & (s >= limit_silence)).sum(), lost.sum()]).tolist()
    return int(vals[0]), int(vals[1]), int(vals[2])
