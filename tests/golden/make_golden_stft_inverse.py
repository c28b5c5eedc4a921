#!/usr/bin/env python3
"""Golden STFT synthesis, bias removal and Griffin-Lim from the reference's own stft.py (:42-141), audio_processing.py
(:7-75) and bias_remover.py (:6-36), imported with the harness stubs of make_golden.py.  librosa is not installed, so its
three helpers the path uses are rebound in the reference's modules: pad_center (a real centre pad), normalize (identity:
the path only calls it with norm=None) and tiny (the smallest normal number of the dtype).  bias_remover.py hard-codes
.cuda(); on this GPU-less box Tensor.cuda and Module.cuda are the identity.

Per configuration (filter_length, hop_length, win_length), on make_golden_stft.waveform() (B = 2, n = 4000):
  env_*      window_sumsquare(...) for the signal's frame count
  basis_*    rows basis_rows_* of inverse_basis (the whole buffer is 4 MB at 1024; the outputs below pin the rest)
  inverse_*  STFT.inverse(*STFT.transform(x));  forward_* STFT.forward(x)
  br09_*, br01_*, bias_*   hifiganBiasRemover(stub_model, ...).forward(x, 0.9 / 0.1) and its bias_spec
  gl_*       (1024 only) two griffin_lim iterations from the stored start angles gl_angles
  err_*      max |fp32 - fp64| of each quantity, the fp64 side from the same classes after .double() (the remover's
             forward casts to float itself, so its fp64 side is its three lines restated on the .double() STFT):
             the tests allow the GPU a multiple of the reference's own rounding error."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402
from make_golden_stft import waveform  # noqa: E402

CONFIGS = {"default": (1024, 256, 1024), "short_window": (512, 128, 400), "small": (64, 16, 64)}


def stub_model(mel):
    """A fixed affine map mel [1, 80, 88] -> audio [1, 1, 88 * 256]: seeded noise plus a per-frame weighted sum of the mel."""
    g = np.random.Generator(np.random.PCG64(5))
    c = torch.from_numpy(g.normal(size=88 * 256).astype(np.float32)).to(mel)
    w = torch.from_numpy((g.normal(size=80) / 80).astype(np.float32)).to(mel)
    return (c + (mel[0] * w[:, None]).sum(0).repeat_interleave(256)).view(1, 1, -1)


def basis_rows(cutoff):
    return np.unique(np.concatenate([np.arange(0, 2 * cutoff, max(1, 2 * cutoff // 10)), [cutoff - 1, cutoff, 2 * cutoff - 1]]))


def main():
    import_reference()
    import librosa.util as lu

    def pad_center(data, size, **k):
        n = data.shape[-1]
        lpad = (size - n) // 2
        return np.pad(data, (lpad, size - n - lpad), mode="constant")

    def normalize(s, norm=None, **k):
        assert norm is None
        return s

    def tiny(x):
        return np.finfo(np.asarray(x).dtype).tiny
    lu.pad_center, lu.normalize, lu.tiny = pad_center, normalize, tiny
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    import audio_processing as ref_ap
    import stft as ref_stft
    ref_stft.pad_center, ref_stft.tiny = pad_center, tiny
    import bias_remover as ref_br

    x = torch.from_numpy(waveform())
    out = {}
    err = lambda a, b: np.float64((a.double() - b).abs().max().item())
    for name, (fl, hop, win) in CONFIGS.items():
        s32, s64 = ref_stft.STFT(fl, hop, win), ref_stft.STFT(fl, hop, win).double()
        mag, ph = s32.transform(x)
        mag64, ph64 = s64.transform(x.double())
        nf = mag.shape[-1]
        out[f"cfg_{name}"] = np.array([fl, hop, win])
        out[f"env_{name}"] = ref_ap.window_sumsquare("hann", nf, hop_length=hop, win_length=win, n_fft=fl, dtype=np.float32)
        rows = basis_rows(fl // 2 + 1)
        out[f"basis_rows_{name}"] = rows
        out[f"basis_{name}"] = s32.inverse_basis[rows, 0, :].numpy()
        out[f"basis_max_{name}"] = np.float32(s32.inverse_basis.abs().max().item())
        inv, inv64 = s32.inverse(mag, ph), s64.inverse(mag64, ph64)
        fwd, fwd64 = s32.forward(x), s64.forward(x.double())
        out[f"inverse_{name}"], out[f"err_inverse_{name}"] = inv.numpy(), err(inv, inv64)
        out[f"forward_{name}"], out[f"err_forward_{name}"] = fwd.numpy(), err(fwd, fwd64)
        br = ref_br.hifiganBiasRemover(stub_model, filter_length=fl, n_overlap=fl // hop, win_length=win)
        out[f"bias_{name}"] = br.bias_spec.numpy()
        bias64 = s64.transform(stub_model(torch.zeros(1, 80, 88, dtype=torch.float64)).squeeze(0))[0][:, :, 0][:, :, None]
        for tag, strength in (("br09", 0.9), ("br01", 0.1)):
            y = br(x, strength)
            y64 = s64.inverse(torch.clamp(mag64 - bias64 * strength, 0.0), ph64)
            out[f"{tag}_{name}"], out[f"err_{tag}_{name}"] = y.numpy(), err(y, y64)
        assert (out[f"br09_{name}"] - out[f"forward_{name}"]).__abs__().max() > 0.1, "the bias must matter"
        if name == "default":
            g = np.random.Generator(np.random.PCG64(17))
            angles = np.angle(np.exp(2j * np.pi * g.random(mag.shape))).astype(np.float32)
            out["gl_angles"] = angles

            def gl(stft, m, a):          # audio_processing.py:70-75 with the drawn angles given
                sig = stft.inverse(m, a).squeeze(1)
                for _ in range(2):
                    _, a = stft.transform(sig)
                    sig = stft.inverse(m, a).squeeze(1)
                return sig
            # the reference's own function, its np.random.rand replaced by the stored draw
            rand = np.random.rand
            np.random.rand = lambda *shape: g2.random(shape)
            g2 = np.random.Generator(np.random.PCG64(17))
            try:
                sig = ref_ap.griffin_lim(mag, s32, n_iters=2)
            finally:
                np.random.rand = rand
            assert torch.equal(sig, gl(s32, mag, torch.from_numpy(angles)))
            out["gl_default"], out["err_gl_default"] = sig.numpy(), err(sig, gl(s64, mag64, torch.from_numpy(angles).double()))
    path = os.path.join(HERE, "stft_inverse.npz")
    np.savez_compressed(path, **out)
    print("wrote stft_inverse.npz", os.path.getsize(path), "bytes")
    for k, v in out.items():
        print(k, v.shape if v.ndim else float(v))


if __name__ == "__main__":
    main()
