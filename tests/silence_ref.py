"""The reference's silence trim (remove_silence.py:7-36, best_checkpoint.py:319-333 and :495-520), restated for the tests.

pydub is not installed, so this is not pydub: it is a restatement of the arithmetic its AudioSegment does under the
reference's loop, for mono 16-bit audio, taken literally from the rules in include/t2amd.h: a segment holding the int16
bytes, len() in rounded milliseconds, slicing by milliseconds with zero fill, audioop.rms, math.log10, the reference's loop
verbatim, the reversal and the final slice.  It decides through the floating-point level, as the reference does, and never
through the integer comparison S < n * R^2 that csrc/silence.hip uses: that comparison is what the tests check."""
import bisect
import math
import warnings

import numpy as np

try:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        import audioop
except ImportError:                                          # removed from the standard library in 3.13
    audioop = None

MAX_AMPLITUDE = 32768.0                                      # max_possible_amplitude of a 16-bit segment
WIDTH = 2                                                    # bytes per frame: mono, 16 bit


def rms_of(data):
    """audioop.rms(data, 2): (unsigned) sqrt(sum x^2 / n) with a double sum, 0 for no frames."""
    if audioop is not None:
        return audioop.rms(data, WIDTH)
    x = np.frombuffer(data, dtype="<i2").astype(np.int64)
    return 0 if x.size == 0 else math.isqrt(int((x * x).sum()) // x.size)


class Segment:
    """A mono 16-bit AudioSegment: the bytes and the frame rate."""

    def __init__(self, data, rate):
        self.data = bytes(data)
        self.rate = int(rate)

    @classmethod
    def from_samples(cls, samples, rate):
        return cls(np.ascontiguousarray(np.asarray(samples), dtype="<i2").tobytes(), rate)

    def samples(self):
        return np.frombuffer(self.data, dtype="<i2").astype(np.int16)

    def frame_count(self):
        return len(self.data) // WIDTH

    def __len__(self):
        return round(1000 * (float(self.frame_count()) / self.rate))

    def _frame(self, ms):
        return int(ms * (self.rate / 1000.0))

    def __getitem__(self, ms):
        assert isinstance(ms, slice) and ms.step is None
        start = 0 if ms.start is None else ms.start
        end = len(self) if ms.stop is None else ms.stop
        assert start >= 0 and end >= 0
        start, end = min(start, len(self)), min(end, len(self))
        fa, fb = self._frame(start), self._frame(end)
        data = self.data[fa * WIDTH:fb * WIDTH] if fb > fa else b""
        missing = (fb - fa) - len(data) // WIDTH
        if missing > 0:                                      # the data ended before fb: zero frames up to fb
            assert missing <= self._frame(2), "more than 2 ms missing: pydub raises TooManyMissingFrames"
            data += b"\0" * (missing * WIDTH)
        return Segment(data, self.rate)

    @property
    def rms(self):
        return rms_of(self.data)

    @property
    def dBFS(self):
        rms = self.rms
        if rms == 0:
            return -float("inf")
        return 20 * math.log10(rms / MAX_AMPLITUDE)

    def reverse(self):
        return Segment(self.samples()[::-1].tobytes(), self.rate)


def detect_leading_silence(sound, silence_threshold=-50.0, chunk_size=10):
    """remove_silence.py:7-20, verbatim."""
    trim_ms = 0  # ms
    while sound[trim_ms:trim_ms+chunk_size].dBFS < silence_threshold:
        trim_ms += chunk_size
        if trim_ms > len(sound):
            return None

    return trim_ms


def trim(samples, rate=22050, silence_threshold=-50.0, chunk_size=10):
    """remove_silence.py:27-35 on an int16 array: (trimmed int16 array, start_trim, end_trim), or (None, None, None) for an
    item the loop skips.  Raises TypeError, as the reference's `duration - None` does, when the start is found and the end is
    not."""
    sound = Segment.from_samples(samples, rate)
    start_trim = detect_leading_silence(sound, silence_threshold, chunk_size)
    if start_trim is None:
        return None, None, None
    end_trim = detect_leading_silence(sound.reverse(), silence_threshold, chunk_size)

    duration = len(sound)
    trimmed_sound = sound[start_trim:duration-end_trim]
    return trimmed_sound.samples(), start_trim, end_trim


def quantise(x):
    """fp32 in int16 units -> int16 as the loader does: NaN -> 0, clamped to the int16 range, truncated toward zero."""
    x = np.asarray(x, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    return np.trunc(np.clip(x, -32768.0, 32767.0)).astype(np.int16)


_levels = None


def threshold_rms(thr):
    """The smallest rms in 1..32768 whose level is not below thr, by the levels themselves; 32769 when every level is below."""
    global _levels
    if _levels is None:
        _levels = [20 * math.log10(k / MAX_AMPLITUDE) for k in range(1, 32769)]
        assert all(a <= b for a, b in zip(_levels, _levels[1:]))      # sorted: the walk from 1 and the bisection find the same rms
    return bisect.bisect_left(_levels, thr) + 1                       # the first level with not (level < thr); 32769 if none
