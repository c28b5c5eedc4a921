"""CPU-only checks of the silence trim: the restatement of silence_ref.py against hand-stated values, the pure host plan of
csrc/silence.hip through the ABI, and the integer decision S < n * R^2 (with the chunk rule the kernels derive from the
reference's loop) against audioop.rms and the loop itself."""
import math
import random

import numpy as np
import pytest
import torch

import silence_ref as R


@pytest.fixture(scope="module")
def L():
    from tacotron2_subword_amd import build
    from tacotron2_subword_amd import _lib
    build.build()
    return _lib


def _seg(n, rate, value=0):
    return R.Segment.from_samples(np.full(n, value, dtype=np.int16), rate)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_chunk_boundaries_at_22050():
    s = _seg(22050, 22050)
    assert [s._frame(10 * k) for k in range(6)] == [0, 220, 441, 661, 882, 1102]
    sizes = [s[10 * k:10 * k + 10].frame_count() for k in range(100)]
    assert set(sizes) == {220, 221} and sum(sizes) == 22050
    fwd = {s._frame(10 * k) for k in range(100)}
    back = {22050 - s._frame(10 * k) for k in range(1, 100)}          # where the reversed sound's chunks begin, in forward frames
    assert 220 in fwd and 220 not in back and 221 in back and 221 not in fwd      # the two grids do not coincide:
    assert len(fwd & back) == 49                                      # only the exact boundaries, every 20 ms, are shared


def test_len_rounds_half_to_even():
    assert len(_seg(8, 16000)) == 0                                   # 0.5 ms -> 0
    assert R.trim(np.full(8, 30000, dtype=np.int16), 16000) == (None, None, None)
    assert len(_seg(24, 16000)) == 2                                  # 1.5 ms -> 2
    assert len(_seg(40, 16000)) == 2                                  # 2.5 ms -> 2
    s = _seg(66161, 22050, 1000)
    assert len(s) == 3000 and s._frame(3000) == 66150
    out, start, end = R.trim(s.samples(), 22050)
    assert (start, end, len(out)) == (0, 0, 66150)


def test_zero_fill_when_len_rounds_up():
    s = _seg(24, 16000, 5000)                                         # 2 ms = 32 frames of which 24 exist
    piece = s[0:10]
    assert piece.frame_count() == 32 and (piece.samples()[:24] == 5000).all() and (piece.samples()[24:] == 0).all()
    out, start, end = R.trim(s.samples(), 16000)
    assert (start, end) == (0, 0) and len(out) == 32 and (out[24:] == 0).all()
    assert s[5:3].frame_count() == 0 and s[7:9].frame_count() == 0    # b <= a, and both ends clamped to len


def test_levels():
    assert _seg(0, 22050).dBFS == -math.inf and _seg(100, 22050).dBFS == -math.inf
    assert _seg(220, 22050, 103).dBFS < -50.0 <= _seg(220, 22050, 104).dBFS
    assert _seg(220, 22050, -32768).dBFS == 0.0
    assert R.detect_leading_silence(_seg(2205, 22050, 103)) is None
    assert R.detect_leading_silence(_seg(2205, 22050, 104)) == 0
    assert R.detect_leading_silence(_seg(0, 22050), -math.inf) == 0   # nothing is below -inf, not even the empty chunk


def test_end_not_found_raises_as_the_reference_does():
    n = next(n for n in range(2205, 9000) if _case_end_none(n) is not None)
    with pytest.raises(TypeError):
        R.trim(_case_end_none(n), 22050)


def _case_end_none(n, rate=22050, chunk=10, amp=104):
    """n frames whose first chunk is exactly loud and which, reversed, end in that chunk plus appended zeros (silent): or None
    when n has no such shape."""
    s = _seg(n, rate)
    ms = len(s)
    if ms % chunk or s._frame(ms) <= n or s._frame(chunk) != n - s._frame(ms - chunk):
        return None
    x = np.zeros(n, dtype=np.int16)
    x[:s._frame(chunk)] = amp
    return x


# ---------------------------------------------------------------------------------------------------------------- the plan
def test_plan_threshold_rms(L):
    for i in range(-900, 1):
        thr = i / 10
        assert L.silence_plan(22050, 10, thr, 1000).R == R.threshold_rms(thr), thr
    assert [L.silence_plan(22050, 10, t, 1000).R for t in (-50.0, -40.0, -60.0)] == [104, 328, 33]
    for k in (1, 2, 33, 104, 328, 1000, 20000, 32767, 32768):        # at a level itself: not below, hence loud
        thr = 20 * math.log10(k / 32768)
        assert L.silence_plan(22050, 10, thr, 1000).R == k == R.threshold_rms(thr)
        assert L.silence_plan(22050, 10, math.nextafter(thr, math.inf), 1000).R == k + 1
    assert L.silence_plan(22050, 10, -math.inf, 1000).R == L.SILENCE_NONE_SILENT == 0
    assert L.silence_plan(22050, 10, -1000.0, 1000).R == 1
    assert L.silence_plan(22050, 10, 0.0, 1000).R == 32768
    assert L.silence_plan(22050, 10, 0.5, 1000).R == L.silence_plan(22050, 10, math.inf, 1000).R == L.SILENCE_ALL_SILENT == 32769


@pytest.mark.parametrize("rate,chunk,n,B", [(22050, 10, 66161, 5), (16000, 7, 24, 1), (16000, 10, 8, 2), (22050, 10, 0, 3), (44100, 25, 100000, 64),
                                            (4000, 1, 17, 1)])
def test_plan_values(L, rate, chunk, n, B):
    p = L.silence_plan(rate, chunk, -50.0, n, B)
    ms = len(_seg(n, rate))
    assert p.len_ms == ms and p.chunks == -(-ms // chunk) and p.chunks_per_group == 8 and p.block == 256
    assert p.out_width == n + int(0.5 * (rate / 1000.0)) + 1 >= _seg(n, rate)._frame(ms)
    assert list(p.scan_grid) == [-(-p.chunks // 8), B, 2] and list(p.cut_grid) == [-(-(p.out_width + 3) // 1024), B]
    assert p.scratch_bytes == 2 * B * 128                           # a cache line per direction and item
    assert L.silence_plan(rate, chunk, -math.inf, n, B).scan_grid[0] == 0


@pytest.mark.parametrize("args,words", [
    ((3999, 10, -50.0, 100, 1), r"sample_rate=3999 outside"),
    ((22050, 0, -50.0, 100, 1), r"chunk_ms=0 outside"),
    ((22050, 10, math.nan, 100, 1), r"threshold_db is NaN"),
    ((22050, 10, -50.0, -1, 1), r"n=-1 samples per row is negative"),
    ((22050, 10, -50.0, 2 ** 30, 1), r"n=1073741824 samples per row exceed"),
    ((22050, 10, -50.0, 100, 0), r"B=0 outside"),
])
def test_plan_refusals(L, args, words):
    with pytest.raises(RuntimeError, match=words):
        L.silence_plan(*args)
    assert L.silence_plan(22050, 10, -50.0, 2 ** 30 - 1, 1).out_width == 2 ** 30 + 11


def test_cpu_tensors_are_refused(L):
    from tacotron2_subword_amd import remove_silence as RS
    x = torch.zeros(2, 100, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        RS.trim_silence(x)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        RS.detect_leading_silence(x[0])
    with pytest.raises(RuntimeError, match="int16"):
        RS.trim_silence(x.double())
    assert RS.silence_stats(torch.tensor([0, 30, -1, 3000, 4000, -1, 10], dtype=torch.int32)) == (7040, 2, 2)
    assert RS.silence_stats(torch.tensor([0, 30, -1]), 30, end_ms=torch.tensor([-1, 0, -1])) == (30, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- the integer decision
def _silent_int(x, n, Rms):
    """What the scan kernel decides for a chunk of n frames whose data is x (the appended zeros are in n only)."""
    x = np.asarray(x, dtype=np.int64)
    return int((x * x).sum()) < n * Rms * Rms


def test_integer_decision_against_audioop():
    rng = random.Random(5)
    nrng = np.random.default_rng(5)
    for thr in (-33.3, -40.0, -50.0, -60.0):
        Rms = R.threshold_rms(thr)
        for it in range(3000):
            n = rng.randint(1, 232)
            kind = it % 6
            if kind < 3:
                x = np.full(n, (Rms - 1, Rms, Rms + 1)[kind], dtype=np.int64) * nrng.choice([-1, 1], n)
            elif kind == 3:
                x = nrng.integers(-2 * Rms, 2 * Rms + 1, n)
            elif kind == 4:
                x = nrng.integers(-32768, 32768, n)
            else:                                                     # at the edge, one sample off
                x = np.full(n, Rms, dtype=np.int64)
                x[rng.randrange(n)] += rng.choice([-1, 1])
            fill = rng.randint(0, 3)                                  # appended zero frames
            seg = R.Segment.from_samples(np.concatenate([x, np.zeros(fill, dtype=np.int64)]), 22050)
            S = int((x * x).sum())
            assert seg.rms == math.isqrt(S // (n + fill))
            assert (seg.dBFS < thr) == _silent_int(x, n + fill, Rms), (thr, n, fill, kind)


def _trim_int(x, rate, thr, chunk):
    """The kernels' arithmetic in Python integers: first loud chunk k with chunk * k < len_ms per direction, then the cut."""
    N = len(x)
    r = rate / 1000.0
    ms = round(1000 * (float(N) / rate))
    Rms = 0 if thr == -math.inf else R.threshold_rms(thr)

    def first(data):
        k = 0
        while chunk * k < ms:
            fa, fb = int(chunk * k * r), int(min(chunk * k + chunk, ms) * r)
            if not _silent_int(data[min(fa, N):min(fb, N)], fb - fa, Rms):
                return chunk * k
            k += 1
        return -1

    start, end = (0, 0) if Rms == 0 else (first(x), first(x[::-1]))
    if start < 0:
        return None, -1, -1
    if end < 0:
        return None, start, -1
    fa, fb = int(start * r), int((ms - end) * r)
    out = np.zeros(max(fb - fa, 0), dtype=np.int16)
    live = x[fa:min(fb, N)] if fb > fa else x[:0]
    out[:len(live)] = live
    return out, start, end


def test_integer_trim_against_the_loop():
    rng = np.random.default_rng(11)
    for it in range(300):
        rate, chunk = [(22050, 10), (16000, 10), (22050, 7), (16000, 7), (8000, 3)][it % 5]
        thr = (-50.0, -40.0, -60.0, -math.inf)[it % 4] if it % 7 else 1.0
        N = int(rng.integers(0, 3000))
        x = rng.integers(-40, 41, N).astype(np.int16)
        if it % 3 and N:
            a = int(rng.integers(0, N))
            b = int(rng.integers(a, min(N, a + 600) + 1))
            x[a:b] = rng.integers(-3000, 3001, b - a)
        got, gs, ge = _trim_int(x, rate, thr, chunk)
        try:
            want, ws, we = R.trim(x, rate, thr, chunk)
        except TypeError:
            assert got is None and gs >= 0 and ge == -1
            continue
        if want is None:
            assert got is None and (gs, ge) == (-1, -1)
        else:
            assert (gs, ge) == (ws, we) and np.array_equal(got, want), (it, rate, chunk, thr, N)
