"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the log-mel front end (`oracle/conformer_ref.py::log_mel_features`, which
casts to float32 internally) with every knob of the C entry points `mi355x_logmel_fwd` / `mi355x_feat_normalize` as a parameter,
for tests/test_frontend_host.py and tests/test_frontend_gpu.py.

  dither        x[t] + dither * noise[t]                                   (explicit noise, features.py:435-436)
  pre-emphasis  y[0] = x[0], y[t] = x[t] - preemph * x[t-1]; y[t] = 0 for t >= audio_len        (:439-442)
  framing       frame f covers samples f * hop - n_fft/2 ... + n_fft (zeros outside [0, S)), T = 1 + S // hop frames
  window        any length <= n_fft, zero-padded to n_fft with (n_fft - win) // 2 zeros in front (torch.stft's rule)
  power         |rfft|^2, n_fft/2 + 1 bins;  mel = fb @ power;  raw = log(mel + log_guard)
  normalise     per (utterance, filter) over frames t < seq_len: mean, unbiased std (NaN -> 0), (x - mean) / (std + 1e-5); frames
                t >= seq_len hold pad_value; the frame axis is padded to a multiple of pad_to with pad_value

Everything runs in `dtype` (float64 by default).  The float32 evaluation of the same code (dtype=torch.float32) is what the GPU
tests measure their tolerance with: its distance from the float64 result is the error a correct float32 front end makes.
The arguments are used as given: a caller that compares with a float32 kernel passes the float32-rounded `preemph`."""
from __future__ import annotations

import torch
import torch.nn.functional as F

STD_EPS = 1e-5


def seq_len(audio_len, hop, n_fft=512):
    """frames the reference counts as valid (features.py:413-417 with centre padding): audio_len // hop, and 0 for an empty clip"""
    n = torch.div(audio_len + 2 * (n_fft // 2) - n_fft, hop, rounding_mode="floor").long()
    return torch.where(audio_len == 0, torch.zeros_like(n), n)


def preemphasised(audio, audio_len, preemph=0.97, noise=None, dither=0.0, dtype=torch.float64):
    """[B, S] -> dithered, pre-emphasised, length-masked signal in `dtype`"""
    x = audio.to(dtype)
    if dither > 0 and noise is not None:
        x = x + dither * noise.to(dtype)
    y = torch.cat([x[:, :1], x[:, 1:] - preemph * x[:, :-1]], dim=1) if preemph else x
    t = torch.arange(x.shape[1]).unsqueeze(0)
    return torch.where(t < audio_len.unsqueeze(1), y, torch.zeros_like(y))


def padded_window(window, n_fft=512, dtype=torch.float64):
    win = window.numel()
    assert 0 < win <= n_fft
    w = torch.zeros(n_fft, dtype=dtype)
    off = (n_fft - win) // 2
    w[off: off + win] = window.to(dtype)
    return w


def power_spectrum(y, window, hop, n_fft=512):
    """y [B, S] (already pre-emphasised and masked) -> [B, T, n_fft/2 + 1] by explicit framing, T = 1 + S // hop"""
    B, S = y.shape
    T = 1 + S // hop
    yp = F.pad(y, (n_fft // 2, n_fft // 2))
    idx = (torch.arange(T) * hop).unsqueeze(1) + torch.arange(n_fft).unsqueeze(0)
    frames = yp[:, idx] * padded_window(window, n_fft, y.dtype)
    spec = torch.fft.rfft(frames, n=n_fft, dim=-1)
    return spec.real ** 2 + spec.imag ** 2


def log_mel(audio, audio_len, fb, window, hop, n_fft=512, preemph=0.97, log_guard=2.0 ** -24, noise=None, dither=0.0,
            dtype=torch.float64):
    """what `mi355x_logmel_fwd` computes: raw log-mel [B, n_mels, T] over ALL T = 1 + S // hop frames (no masking of frames)"""
    y = preemphasised(audio, audio_len, preemph, noise, dither, dtype)
    power = power_spectrum(y, window, hop, n_fft)
    fbt = fb.reshape(-1, n_fft // 2 + 1).to(dtype)
    mel = torch.matmul(power, fbt.t()).transpose(1, 2)
    return torch.log(mel + torch.tensor(log_guard, dtype=dtype))


def feat_normalize(raw, n_frames, normalize=True, pad_value=0.0, pad_to=0):
    """what `mi355x_feat_normalize` computes (in raw's dtype), plus the module's `pad_to`"""
    B, _, T = raw.shape
    n_frames = torch.clamp(n_frames, max=T)
    tmask = (torch.arange(T).unsqueeze(0) < n_frames.unsqueeze(1)).unsqueeze(1)
    feat = raw
    if normalize:
        n = n_frames.to(raw.dtype).view(B, 1)
        zero = torch.zeros_like(raw)
        mean = torch.where(tmask, raw, zero).sum(2) / n
        var = (torch.where(tmask, raw - mean.unsqueeze(2), zero) ** 2).sum(2) / (n - 1.0)
        std = torch.sqrt(var)
        std = torch.where(torch.isnan(std), torch.zeros_like(std), std) + STD_EPS
        feat = (raw - mean.unsqueeze(2)) / std.unsqueeze(2)
    feat = torch.where(tmask, feat, torch.full_like(feat, pad_value))
    if pad_to > 0 and T % pad_to:
        feat = F.pad(feat, (0, pad_to - T % pad_to), value=pad_value)
    return feat


def log_mel_features(audio, audio_len, fb, window, hop, n_fft=512, preemph=0.97, log_guard=2.0 ** -24, noise=None, dither=0.0,
                     normalize=True, pad_value=0.0, pad_to=0, dtype=torch.float64):
    """the whole front end, = `conformer_ref.log_mel_features` in `dtype`: (features [B, n_mels, T (padded)], seq_len [B]);
    `normalize`: True / "per_feature", anything else leaves the valid frames as they are"""
    raw = log_mel(audio, audio_len, fb, window, hop, n_fft, preemph, log_guard, noise, dither, dtype)
    n = seq_len(audio_len, hop, n_fft)
    return feat_normalize(raw, n, normalize is True or normalize == "per_feature", pad_value, pad_to), n
