"""GPU checks of the silence trim (csrc/silence.hip, remove_silence.py): every item bit for bit against the restatement of
silence_ref.py (trimmed samples, length, start_ms, end_ms), at the smallest shapes that can go wrong."""
import math

import numpy as np
import pytest
import torch

import silence_ref as R

pytestmark = pytest.mark.gpu

GARBAGE = 30000          # what lies behind every item's length in a padded batch: loud, so that reading it shows
_ref_cache = {}


def _RS():
    from tacotron2_subword_amd import remove_silence as RS
    return RS


def _ref(x, rate, thr, chunk):
    """The restatement's (trimmed, start, end); (None, -1, -1) for a skipped item; (None, start, -1) where the reference raises."""
    key = (x.tobytes(), rate, thr, chunk)
    if key not in _ref_cache:
        try:
            out, s, e = R.trim(x, rate, thr, chunk)
            _ref_cache[key] = (out, -1, -1) if out is None else (out, s, e)
        except TypeError:
            _ref_cache[key] = (None, R.detect_leading_silence(R.Segment.from_samples(x, rate), thr, chunk), -1)
    return _ref_cache[key]


def _pad(items, extra=37, dtype=np.int16):
    n = max(len(x) for x in items) + extra
    batch = np.full((len(items), n), GARBAGE, dtype=dtype)
    for i, x in enumerate(items):
        batch[i, :len(x)] = x
    return batch


def _check(items, got, rate=22050, thr=-50.0, chunk=10):
    out, new, start, end = (t.cpu().numpy() for t in got)
    n = max(len(x) for x in items)
    assert out.shape[1] >= n + int(0.5 * rate / 1000.0) + 1
    for i, x in enumerate(items):
        want, ws, we = _ref(np.asarray(x, dtype=np.int16), rate, thr, chunk)
        what = (i, len(x), rate, thr, chunk)
        assert (int(start[i]), int(end[i])) == (ws, we), what
        assert int(new[i]) == (0 if want is None else len(want)), what
        if want is not None:
            assert np.array_equal(out[i, :len(want)], want), what
        assert not out[i, int(new[i]):].any(), what               # zero behind the new length
    return out, new, start, end


def _trim(items, rate=22050, thr=-50.0, chunk=10, lengths="tensor", **kw):
    batch = torch.from_numpy(_pad(items)).cuda()
    lens = [len(x) for x in items]
    if lengths == "tensor":
        lens = torch.tensor(lens, dtype=torch.int32).cuda()
    return _RS().trim_silence(batch, lens, rate, thr, chunk, **kw)


def _burst(n, a, b, seed=0, quiet=40, loud=3000):
    """n frames of noise below every threshold used here, loud in [a, b)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-quiet, quiet + 1, n).astype(np.int16)
    a, b = min(a, n), min(b, n)
    x[a:b] = rng.integers(-loud, loud + 1, max(b - a, 0))
    return x


@pytest.mark.parametrize("chunk", [10, 7])
@pytest.mark.parametrize("rate", [22050, 16000])
def test_chunk_grid(rate, chunk):
    rng = np.random.default_rng(rate + chunk)
    per_ms = rate // 1000
    sizes = [0, 1, 8, 24, 219, 220, 221, 10 * chunk * rate // 1000, 10 * chunk * rate // 1000 + 1, 4410, 4411, 1600, 1607, 7 * per_ms * 31 + 5]
    items = []
    for n in sizes:
        items.append(rng.integers(-3000, 3001, n).astype(np.int16))                      # loud everywhere
        a = int(rng.integers(0, n + 1))
        items.append(_burst(n, a, min(n, a + int(rng.integers(1, 500))), seed=n))         # loud somewhere
    _check(items, _trim(items, rate, -50.0, chunk), rate, -50.0, chunk)


def test_threshold_edge():
    n = 2205
    items = [np.full(n, v, dtype=np.int16) for v in (103, 104, -103, -104, -32768, 32767, 0)]
    mid = np.full(n, 103, dtype=np.int16)
    mid[882:1102] = 104                                            # exactly chunk 4
    alt = np.full(n, 103, dtype=np.int16)
    alt[441:661:2] = 105                                           # chunk 2: half 105, half 103: rms 104.005
    items += [mid, alt]
    _, new, start, end = _check(items, _trim(items))
    assert start.tolist() == [-1, 0, -1, 0, 0, 0, -1, 40, 20] and new[0] == 0 and new[1] == n
    for thr in (-40.0, -60.0, 20 * math.log10(104 / 32768), math.nextafter(20 * math.log10(104 / 32768), 0.0)):
        _check(items, _trim(items, thr=thr), thr=thr)
    out, new, start, end = _check(items, _trim(items, thr=-math.inf), thr=-math.inf)    # nothing is silent, not even zeros
    assert start.tolist() == [0] * 9 and end.tolist() == [0] * 9 and new.tolist() == [n] * 9
    _, new, start, _ = _check(items, _trim(items, thr=0.5), thr=0.5)                     # everything is
    assert start.tolist() == [-1] * 9 and not new.any()


def _rounds_up(rate, chunk, full_first):
    """The smallest n whose len() is a whole number of chunks and was rounded up, so that the last chunk ends in appended zeros;
    with full_first, the reversed sound's last chunk is, in data, exactly the forward sound's first chunk."""
    for n in range(chunk * rate // 1000, 20000):
        s = R.Segment.from_samples(np.zeros(n, dtype=np.int16), rate)
        ms = len(s)
        if ms % chunk == 0 and s._frame(ms) > n and (not full_first or s._frame(chunk) == n - s._frame(ms - chunk)):
            return n, s._frame(ms - chunk), s._frame(ms)
    raise AssertionError("no such length")


@pytest.mark.parametrize("rate,chunk", [(22050, 10), (16000, 7)])
def test_zero_fill_changes_a_decision(rate, chunk):
    n, fa, fb = _rounds_up(rate, chunk, False)
    m, p = n - fa, fb - n
    assert m >= 1 and p >= 1
    last = np.zeros(n, dtype=np.int16)
    last[fa:] = 104                                                # m * R^2 < (m + p) * R^2: silent with the fill, loud without
    louder = np.zeros(n, dtype=np.int16)
    louder[fa:] = 104 + 1 + int(104 * (math.sqrt((m + p) / m) - 1))   # loud even with the fill
    assert m * int(louder[-1]) ** 2 >= (m + p) * 104 ** 2
    items = [last, louder, last[::-1].copy(), louder[::-1].copy()]
    _, new, start, end = _check(items, _trim(items, rate, -50.0, chunk), rate, -50.0, chunk)
    assert start[0] == -1 and start[1] == len(R.Segment.from_samples(last, rate)) - chunk and end[1] == 0
    # the same in the reversed direction, with the start found: the first chunk exactly loud, the reversed last chunk its data
    # plus appended zeros.  The reference raises on `duration - None`; the item is dropped with its start kept.
    if rate % 1000 == 0:
        return                                                     # whole frames per ms: a rounded-up last chunk is never a full one
    n2, fa2, fb2 = _rounds_up(rate, chunk, True)
    head = np.zeros(n2, dtype=np.int16)
    head[:n2 - fa2] = 104
    with pytest.raises(TypeError):
        R.trim(head, rate, -50.0, chunk)
    _, new, start, end = _check([head], _trim([head], rate, -50.0, chunk), rate, -50.0, chunk)
    assert (int(start[0]), int(end[0]), int(new[0])) == (0, -1, 0)


def test_loud_position_and_empty_results():
    items = []
    for n in (4400, 4410, 4411):                                   # len() rounded up, exact, rounded down
        first, last = np.zeros(n, dtype=np.int16), np.zeros(n, dtype=np.int16)
        first[0], last[-1] = 32767, -32768
        items += [first, last, np.full(n, 5000, dtype=np.int16), np.zeros(n, dtype=np.int16), np.full(n, 50, dtype=np.int16)]
    out, new, start, end = _check(items, _trim(items))
    assert (int(start[2]), int(end[2]), int(new[2])) == (0, 0, 4410) and not out[2, 4400:].any()   # longer than its 4400 frames
    assert (int(start[0]), int(end[0])) == (0, 190)
    assert int(start[11]) == -1                                    # frame 4410 of 4411 lies behind len() = 200 ms: never looked at
    for i in (3, 4, 8, 9, 13, 14):
        assert (int(start[i]), int(end[i]), int(new[i])) == (-1, -1, 0)


def test_long_head_crosses_workgroups():
    from tacotron2_subword_amd import _lib as L
    n = 88200
    x = _burst(n, 66150, 66650, seed=3)                            # loud from chunk 300 on
    y = _burst(n, 66149, 66150, seed=4, loud=32767)
    y[66149] = 32767                                               # one sample, the last of chunk 299
    assert 300 // L.silence_plan(22050, 10, -50.0, n, 2).chunks_per_group > 1
    _, new, start, end = _check([x, y], _trim([x, y]))
    assert start.tolist() == [3000, 2990]
    single = _RS().detect_leading_silence(torch.from_numpy(x).cuda())
    assert single == 3000 and isinstance(single, int)
    assert _RS().detect_leading_silence(torch.zeros(500, dtype=torch.int16).cuda()) is None
    both = _RS().detect_leading_silence(torch.from_numpy(np.stack([x, y[::-1]])).cuda())
    assert both.dtype == torch.int32 and both.tolist() == [3000, int(end[1])]


def test_ragged_batch():
    sizes = [0, 1, 219, 4411, 66161]
    items = [_burst(n, n // 3, n // 3 + 300, seed=n) for n in sizes]
    items[1][0] = 20000
    got = _trim(items, lengths="tensor")
    _check(items, got)
    as_list = _trim(items, lengths="list")
    for a, b in zip(got, as_list):
        assert torch.equal(a, b)
    for i, x in enumerate(items):                                  # each item alone: no lengths, no padding
        alone = _RS().trim_silence(torch.from_numpy(x).cuda().unsqueeze(0))
        k = int(alone[1][0])
        assert k == int(got[1][i]) and int(alone[2][0]) == int(got[2][i]) and int(alone[3][0]) == int(got[3][i])
        assert torch.equal(alone[0][0, :k], got[0][i, :k])
    one = _RS().trim_silence(torch.from_numpy(items[3]).cuda())    # 1-D in, 1-D out
    assert one[0].dim() == 1 and torch.equal(one[0][:int(one[1])], got[0][3, :int(got[1][3])])
    stats = _RS().silence_stats(got[2], limit_silence=60)
    s = got[2].tolist()
    assert stats == (sum(v for v in s if v >= 0), sum(v >= 60 for v in s), sum(v < 0 for v in s))
    with pytest.raises(RuntimeError, match="exceeds"):
        _RS().trim_silence(torch.zeros(1, 10, dtype=torch.int16).cuda(), [11])


def test_float_input_and_output():
    rng = np.random.default_rng(9)
    n = 4411
    special = np.array([0.9, -0.9, 103.99, -103.99, 104.0, -104.5, 40000.0, -40000.0, np.nan, 32767.9, -32768.9, np.inf, -np.inf], dtype=np.float32)
    a = (rng.standard_normal(n) * 30).astype(np.float32)
    a[1500:2500] = (rng.standard_normal(1000) * 4000).astype(np.float32)
    a[1500:1500 + len(special)] = special
    b = np.full(n, 103.99, dtype=np.float32)                       # truncates to 103: silent throughout
    c = np.full(n, -104.99, dtype=np.float32)                      # truncates to -104: loud throughout
    d = np.zeros(n, dtype=np.float32)
    d[:len(special)] = special                                     # the clamped values and the NaN inside the first chunk
    fl = [a, b, c, d]
    q = [R.quantise(x) for x in fl]
    assert q[3][:len(special)].tolist() == [0, 0, 103, -103, 104, -104, 32767, -32768, 0, 32767, -32768, 32767, -32768]
    xf = torch.from_numpy(_pad(fl, dtype=np.float32)).cuda()
    lens = torch.tensor([n] * 4, dtype=torch.int32).cuda()
    RS = _RS()
    from_float = RS.trim_silence(xf, lens)
    from_int = _trim(q)
    _check(q, from_float)
    for u, v in zip(from_float, from_int):
        assert torch.equal(u, v)
    as_float = RS.trim_silence(xf, lens, out_dtype=torch.float32)
    assert as_float[0].dtype == torch.float32 and torch.equal(as_float[0], from_int[0].float() / 32768)
    for u, v in zip(as_float[1:], from_int[1:]):
        assert torch.equal(u, v)
    scaled = RS.trim_silence(torch.from_numpy(_pad(q)).cuda(), lens, out_dtype=torch.float32, scale=0.5)
    assert torch.equal(scaled[0], from_int[0].float() * 0.5)
    with pytest.raises(RuntimeError, match="scale"):
        RS.trim_silence(xf, lens, scale=0.5)


def test_chain_into_mel_spectrogram():
    from tacotron2_subword_amd import stft as S
    front = S.TacotronSTFT().cuda()
    rng = np.random.default_rng(21)
    items = []
    for i, (head, body, tail) in enumerate([(700, 6615, 1300), (0, 7000, 2205), (3000, 6000, 0), (441, 8000, 450)]):
        x = rng.integers(-20, 21, head + body + tail).astype(np.int16)
        t = np.arange(body)
        x[head:head + body] = (9000 * np.sin(t * (0.05 + 0.01 * i)) + rng.integers(-500, 501, body)).astype(np.int16)
        items.append(x)
    trimmed, new, start, end = _trim(items, out_dtype=torch.float32)
    _check(items, (torch.round(trimmed * 32768).to(torch.int16), new, start, end))
    mel, frames = front.mel_spectrogram(trimmed, lengths=new, time_major=True)
    for i, x in enumerate(items):
        want, _, _ = _ref(x, 22050, -50.0, 10)
        alone = front.mel_spectrogram((torch.from_numpy(want).float() / 32768).unsqueeze(0).cuda(), time_major=True)[0]
        nf = alone.shape[0]
        assert int(frames[i]) == nf == 1 + len(want) // 256
        assert torch.equal(mel[i, :nf], alone), i
