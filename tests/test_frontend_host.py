"""CPU: the float64 front-end oracle (tests/frontend_oracle.py) pinned without a GPU -- against `conformer_ref.log_mel_features`
(float32; tied to the reference-made fixture by test_oracle_pinning.py) at the recipe geometry and at others, against
`torch.stft(center=True, pad_mode="constant")` in float64 (the call the reference front end is built on; independent of the
explicit framing in the oracle), and on the frame counts for every hop.

Bounds.  Against the float32 reference: 1e-3, the project's contract for front-end features (log-mel values lie in [-16.7, 0] for
0.1-sigma audio; the float32 evaluation of the oracle itself sits 2e-5 .. 1.5e-4 from the float64 one).  Against torch.stft in
float64: 1e-10 on power spectra of O(1..100) (measured 3e-14: both sides are one 512-point FFT in float64)."""
import numpy as np
import pytest
import torch

from oracle import conformer_ref as R

import frontend_oracle as FO


def _fb(sr, n_mels):
    from nemo_amd.modules.audio_preprocessing import slaney_mel_filterbank
    return torch.from_numpy(slaney_mel_filterbank(sr, 512, n_mels, 0.0, sr / 2.0, "slaney"))


def _batch(S, seed, B=3):
    g = torch.Generator().manual_seed(seed)
    audio = 0.1 * torch.randn(B, S, generator=g)
    alen = torch.tensor([S, max(1, S // 3), max(1, S - 161), 0, 1][:B])
    return audio, alen, g


GEOMETRIES = [  # hop, window length, mels, sample rate, samples
    (160, 400, 80, 16000, 16037),
    (200, 400, 80, 16000, 12801),
    (256, 512, 128, 16000, 20002),
    (80, 320, 64, 16000, 9000),
    (220, 441, 80, 22050, 15003),
    (161, 320, 80, 8000, 8000),
    (512, 100, 80, 16000, 33000),
]


def test_recipe_geometry_matches_the_reference_defaults():
    """hop 160, 400-sample Hann, 80 mels: the oracle with the reference's own default filterbank and window"""
    audio, alen, _ = _batch(16037, 1, B=5)
    fb, win = torch.from_numpy(R.mel_filterbank()), R.hann_window_sym(400)
    ref, ref_len = R.log_mel_features(audio, alen)
    got, got_len = FO.log_mel_features(audio, alen, fb, win, 160, preemph=0.97, log_guard=R.LOG_GUARD)
    assert got.dtype == torch.float64 and torch.equal(got_len, ref_len)
    assert torch.isfinite(got).all()
    assert (got - ref.double()).abs().max().item() < 1e-3
    assert np.array_equal(_fb(16000, 80).numpy(), R.mel_filterbank())  # the module's filterbank IS the reference's


@pytest.mark.parametrize("hop,win,n_mels,sr,S", GEOMETRIES)
@pytest.mark.parametrize("normalize", [True, "NA"])
def test_oracle_against_float32_reference(hop, win, n_mels, sr, S, normalize):
    audio, alen, g = _batch(S, hop, B=5)
    fb = _fb(sr, n_mels)
    window = torch.hamming_window(win, periodic=False) if win == 441 else torch.hann_window(win, periodic=False)
    noise = torch.randn(audio.shape, generator=g)
    kw = dict(dither=1e-3, noise=noise, pad_to=16, pad_value=-3.0, normalize=normalize)
    ref, ref_len = R.log_mel_features(audio, alen, fb=fb, window=window, hop=hop, win=win, n_mels=n_mels, preemph=0.9, **kw)
    got, got_len = FO.log_mel_features(audio, alen, fb, window, hop, preemph=0.9, log_guard=R.LOG_GUARD, **kw)
    assert got.shape == ref.shape and got.shape[-1] % 16 == 0 and torch.equal(got_len, ref_len)
    assert (got - ref.double()).abs().max().item() < 1e-3
    # the float32 evaluation of the oracle (the yardstick of the GPU tests' tolerance) is the same computation
    got32, _ = FO.log_mel_features(audio, alen, fb, window, hop, preemph=0.9, log_guard=R.LOG_GUARD, dtype=torch.float32, **kw)
    assert got32.dtype == torch.float32 and (got - got32.double()).abs().max().item() < 1e-3


@pytest.mark.parametrize("hop,win", [(200, 400), (256, 512), (161, 320), (160, 400), (264, 441), (1, 400)])
def test_power_spectrum_against_torch_stft(hop, win):
    S = 700 if hop == 1 else 9001
    audio, alen, _ = _batch(S, 7 * hop + win)
    window = torch.hann_window(win, periodic=False, dtype=torch.float64)
    y = FO.preemphasised(audio, alen, 0.97)
    assert y.dtype == torch.float64
    spec = torch.stft(y, n_fft=512, hop_length=hop, win_length=win, window=window, center=True, pad_mode="constant",
                      return_complex=True)  # [B, 257, T]
    want = (spec.real ** 2 + spec.imag ** 2).transpose(1, 2)
    got = FO.power_spectrum(y, window, hop)
    assert got.shape == want.shape == (3, 1 + S // hop, 257)
    assert want.max().item() > 1.0
    assert (got - want).abs().max().item() < 1e-10


def test_preemphasis_mask_and_knobs():
    audio, alen, g = _batch(50, 3, B=5)
    y = FO.preemphasised(audio, alen, 0.97)
    x = audio.double()
    assert torch.equal(y[0, 0], x[0, 0]) and torch.equal(y[0, 1:], x[0, 1:] - 0.97 * x[0, :-1])
    assert not y[3].any() and y[4, 0] == x[4, 0] and not y[4, 1:].any() and not y[1, 16:].any() and y[1, 15] != 0
    assert torch.equal(FO.preemphasised(audio, alen, 0.0)[0], x[0])
    noise = torch.randn(audio.shape, generator=g)
    yd = FO.preemphasised(audio, alen, 0.0, noise=noise, dither=0.5)
    assert torch.equal(yd[0], x[0] + 0.5 * noise[0].double()) and not yd[3].any()
    # log guard, window shorter than n_fft (centred), filterbank of any height
    w = FO.padded_window(torch.ones(441))
    assert w[:35].sum() == 0 and w[35:476].sum() == 441 and w[476:].sum() == 0
    silent = FO.log_mel(torch.zeros(1, 400), torch.tensor([400]), _fb(16000, 7), torch.ones(100), 100,
                        log_guard=float(torch.finfo(torch.float32).tiny))
    assert silent.shape == (1, 7, 5) and torch.allclose(silent, torch.full_like(silent, float(np.log(np.float64(2.0) ** -126))))


@pytest.mark.parametrize("hop", [1, 80, 160, 161, 200, 220, 256, 264, 512])
def test_sequence_lengths(hop):
    alen = torch.tensor([0, 1, hop - 1, hop, hop + 1, 255, 256, 257, 16000, 16037, 32 * hop, 32 * hop - 1])
    want = R.mel_seq_len(alen, 512, hop)
    want[alen == 0] = 0
    got = FO.seq_len(alen, hop)
    assert torch.equal(got, want) and torch.equal(got, alen // hop) and got[0] == 0
    short = torch.tensor([0, 1, hop - 1, hop, hop + 1, 33 * hop])
    feat, n = FO.log_mel_features(torch.zeros(6, 33 * hop), short, _fb(16000, 8), torch.ones(64), hop)
    assert torch.equal(n, short // hop) and feat.shape == (6, 8, 34)
    # the module counts frames by the same rule, for any hop
    from nemo_amd.modules.audio_preprocessing import FilterbankFeatures
    f = FilterbankFeatures(n_window_size=400, n_window_stride=hop, nfilt=8)
    mod = f.get_seq_len(alen)
    assert torch.equal(torch.where(alen == 0, torch.zeros_like(mod), mod), want)


def test_feat_normalize_edges():
    g = torch.Generator().manual_seed(5)
    raw = torch.randn(5, 7, 9, generator=g, dtype=torch.float64)
    n = torch.tensor([0, 1, 2, 9, 4])
    out = FO.feat_normalize(raw, n, True, pad_value=-1.5, pad_to=4)
    assert out.shape == (5, 7, 12) and torch.isfinite(out).all()
    assert (out[0] == -1.5).all() and (out[1, :, 0] == 0).all() and (out[1, :, 1:] == -1.5).all()
    assert torch.allclose(out[2, :, :2].abs(), torch.full((7, 2), 2 ** -0.5, dtype=torch.float64), atol=1e-4)
    v = raw[3]
    assert torch.allclose(out[3, :, :9], (v - v.mean(1, keepdim=True)) / (v.std(1, keepdim=True) + 1e-5), atol=1e-12)
    assert (out[3, :, 9:] == -1.5).all() and (out[4, :, 4:] == -1.5).all()
    off = FO.feat_normalize(raw, n, False, pad_value=2.0)
    assert torch.equal(off[3], raw[3]) and torch.equal(off[4, :, :4], raw[4, :, :4]) and (off[4, :, 4:] == 2.0).all()
