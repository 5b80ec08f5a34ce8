"""-m gpu: the log-mel front end (csrc/mel.hip: `mi355x_logmel_fwd`, `mi355x_feat_normalize`, and the module on top of them) against
the float64 oracle of tests/frontend_oracle.py over hop, window, mel count, sample rate, filterbank layout, sample count, row
alignment and length edges.  Every raw log-mel case runs ALL THREE kernels (`mi355x_logmel_config(0 / 1 / 2)`), into an output
filled with NaN, and compares every frame and mel bin, the frames beyond the audio length included.

Tolerance of the raw log-mel comparison.  Per case the yardstick is the REFERENCE's own float32 error: `spread` = the largest
absolute difference between the float32 and the float64 evaluation of the oracle on the case's input (0.1-sigma Gaussian audio,
log-mel values in [-16.7, 0], -87.3 with the float32 `tiny` guard).  A kernel may sit TOL_MULT = 4 spreads from the float64
result: its DFT sums in another order than torch.fft's, so its error is another draw of the same size, not the same number.
Measured on an MI355X over the 80 raw cases below x 3 kernels: spread 1.2e-6 (no pre-emphasis, or five wide filters) .. 1.54e-4
(80 mels at 22.05 kHz); worst kernel error 1.93e-4 (128 mels, packed layout, hop 161, round-1 kernel; spread 1.02e-4); worst
error / spread 1.91 (the same case; 1.90 on the register kernel, 128 mels at hop 200).  4 leaves a factor of two over that and
keeps the largest bound at 6.2e-4.
One stale frame is an error of order 1 or more (the register kernel before its staging covered hops above 181: 1.2 at hop 182
with a 512-sample window, 12 .. 68 and non-finite cells at hops 200 .. 264), three orders above the bound.
Normalised features keep the project's contract of 1e-3; bf16 outputs add their rounding, 2^-8 relative.
The file adds about 3 s to the GPU suite (104 tests, 2.8 s measured)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import frontend_oracle as FO

dev = "cuda"
TOL_MULT = 4.0
P97 = float(np.float32(0.97))            # the C entry point takes the coefficient as a float
GUARD = 2.0 ** -24
TINY = float(torch.finfo(torch.float32).tiny)
MI_ERR_ARG = 1


def ops():
    from nemo_amd import ops as _ops
    return _ops


def _fb(sr=16000, n_mels=80):
    from nemo_amd.modules.audio_preprocessing import slaney_mel_filterbank
    return torch.from_numpy(slaney_mel_filterbank(sr, 512, n_mels, 0.0, sr / 2.0, "slaney"))


def _window(kind, n):
    fn = {"hann": torch.hann_window, "hamming": torch.hamming_window}.get(kind)
    return fn(n, periodic=False) if fn else torch.ones(n)


def _layout(fb, kind):
    """(first bin, taps, offset, weights) of a dense [n_mels, 257] filterbank on the device.  "sparse": what the module passes
    (offsets multiples of four, zero fill); "packed": the same spans back to back, offsets not multiples of four, no fill;
    "dense": all 257 taps of every row, more weights than the kernels keep in the LDS"""
    from nemo_amd.modules.audio_preprocessing import sparsify_filterbank
    st, ln, off, w = sparsify_filterbank(fb)
    if kind == "packed":
        rows = [fb[m, int(s): int(s) + int(n)] for m, (s, n) in enumerate(zip(st, ln))]
        off = torch.tensor(np.concatenate([[0], np.cumsum(ln.numpy())[:-1]]), dtype=torch.int32)
        w = torch.cat(rows).float()
        assert (off % 4 != 0).any() and w.numel() == int(ln.sum())
    elif kind == "dense":
        n_mels, nb = fb.shape
        st = torch.zeros(n_mels, dtype=torch.int32)
        ln = torch.full((n_mels,), nb, dtype=torch.int32)
        off = (torch.arange(n_mels) * nb).to(torch.int32)
        w = fb.float().reshape(-1).clone()
        assert w.numel() > 1024
    else:
        assert kind == "sparse" and (off % 4 == 0).all()
    return tuple(t.contiguous().to(dev) for t in (st, ln, off, w))


def _audio(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.1 * torch.randn(B, S, generator=g)


def _three_kernels(run):
    """run(variant) under each of the three kernels; the configuration is restored whatever happens"""
    from nemo_amd._lib import lib
    prev = lib.mi355x_logmel_config(-1)
    outs = []
    try:
        for variant in (0, 1, 2):
            lib.mi355x_logmel_config(variant)
            outs.append(run(variant))
    finally:
        lib.mi355x_logmel_config(prev)
    assert lib.mi355x_logmel_config(-1) == prev
    return outs


def _check_raw(name, audio, alen, fb, window, hop, preemph=P97, guard=GUARD, layout="sparse"):
    """all three kernels against the float64 oracle, every cell; the figures are printed before anything is asserted"""
    o = ops()
    B, S = audio.shape
    n_mels, T = fb.shape[0], 1 + S // hop
    ref = FO.log_mel(audio, alen, fb, window, hop, preemph=preemph, log_guard=guard)
    ref32 = FO.log_mel(audio, alen, fb, window, hop, preemph=preemph, log_guard=guard, dtype=torch.float32)
    assert ref.shape == (B, n_mels, T) and torch.isfinite(ref).all()
    spread = (ref32.double() - ref).abs().max().item()
    assert 0.0 < spread < 1e-3, spread   # (the yardstick itself: a float32 front end is that close to the float64 one)
    a, l, w, sp = audio.to(dev), alen.to(dev), window.float().to(dev), _layout(fb, layout)

    def run(variant):
        out = torch.full((B, n_mels, T), float("nan"), device=dev)
        o.logmel(a, l, w, sp, n_mels, hop=hop, preemph=preemph, log_guard=guard, out=out)
        torch.cuda.synchronize()
        return out.cpu()

    outs = _three_kernels(run)
    errs = []
    for variant, out in enumerate(outs):
        d = (out.double() - ref).abs()
        d = torch.where(torch.isfinite(out), d, torch.full_like(d, float("inf")))
        err = d.max().item()
        bad = int((d > TOL_MULT * spread).sum())
        errs.append(err)
        print(f"[frontend] {name} kernel {variant}: max|err| {err:.3e}  spread {spread:.3e}  ratio {err / spread:.2f}  "
              f"cells over {bad}/{d.numel()}  frames over {sorted(set(torch.nonzero(d > TOL_MULT * spread)[:, 2].tolist()))[:8]}")
    for variant, err in enumerate(errs):
        assert err <= TOL_MULT * spread, (name, variant, err, spread)
    return outs


def _lens(S, B):
    return torch.tensor([S, max(1, S // 3), max(1, S - 161), max(1, S - 1), 1][:B])


# ---------------------------------------------------------------------------------------------- hop
HOPS = [80, 160, 180, 182, 200, 220, 240, 256, 264, 266, 320, 512, 161, 255]


@pytest.mark.parametrize("hop,win", [(h, 400) for h in HOPS] + [(h, 512) for h in (180, 182, 264, 266)])
def test_logmel_hop_sweep(hop, win):
    """T = 71: two full 32-frame blocks and a partial one per row, so the LAST frames of a full block (the ones whose samples lie
    deepest in the staged segment) are compared.  180 / 182: one staging trip of the register kernel ends here; 264 / 266: the
    launcher's limit for that kernel; odd hops take the radix-4 kernel.  The 512-sample window has no zero tail to hide a stale
    sample behind."""
    S = 70 * hop + 37
    _check_raw(f"hop{hop}_win{win}", _audio(3, S, hop), _lens(S, 3), _fb(), _window("hann", win), hop)


def test_logmel_hop_1_short_clip():
    _check_raw("hop1", _audio(3, 300, 1), torch.tensor([300, 100, 299]), _fb(), _window("hann", 400), 1)


# ---------------------------------------------------------------------------------------------- window
@pytest.mark.parametrize("hop", [160, 220])
@pytest.mark.parametrize("win,kind", [(320, "hann"), (400, "hamming"), (441, "hann"), (441, "none"), (512, "hamming"),
                                      (512, "none"), (100, "hann")])
def test_logmel_window_length_and_type(hop, win, kind):
    """odd lengths are centred with the shorter half in front ((512 - win) // 2, torch.stft's rule); 100 < hop: samples between two
    frames' windows are never seen"""
    S = 40 * hop + 2
    _check_raw(f"win{win}_{kind}_hop{hop}", _audio(3, S, win + hop), _lens(S, 3), _fb(), _window(kind, win), hop)


# ---------------------------------------------------------------------------------------------- mel count, sample rate, layout
@pytest.mark.parametrize("n_mels,sr,hop,win", [(64, 16000, 160, 400), (80, 16000, 160, 400), (128, 16000, 160, 400),
                                               (128, 16000, 256, 512), (80, 22050, 220, 441), (80, 8000, 80, 200),
                                               (80, 8000, 200, 400)])
def test_logmel_mel_count_and_sample_rate(n_mels, sr, hop, win):
    S = 45 * hop + 1
    _check_raw(f"mels{n_mels}_sr{sr}_hop{hop}", _audio(3, S, n_mels + sr), _lens(S, 3), _fb(sr, n_mels), _window("hann", win), hop)


@pytest.mark.parametrize("hop", [160, 200, 161])
@pytest.mark.parametrize("layout,n_mels", [("sparse", 80), ("packed", 80), ("packed", 128), ("dense", 80), ("dense", 5)])
def test_logmel_filterbank_layouts(layout, n_mels, hop):
    """packed: `fb_aligned == 0` in the register kernel (scalar weight reads); dense: more than FB_CAP = 1024 weights, which stay in
    global memory (80 x 257 and 5 x 257)"""
    S = 40 * hop + 3
    _check_raw(f"{layout}{n_mels}_hop{hop}", _audio(3, S, 9), _lens(S, 3), _fb(16000, n_mels), _window("hann", 400), hop,
               layout=layout)


# ---------------------------------------------------------------------------------------------- sample count, alignment, lengths
@pytest.mark.parametrize("hop,S", [(160, 16000), (160, 16001), (160, 16002), (160, 16003), (200, 12801), (200, 12802),
                                   (200, 12803), (256, 9000), (160, 331), (200, 150), (160, 2 * 32 * 160), (256, 2 * 32 * 256),
                                   (200, 3 * 32 * 200), (160, 32 * 160 - 1)])
def test_logmel_sample_count_and_row_alignment(hop, S):
    """five rows of S floats: with S mod 4 = 1, 2, 3 the rows start at every 16-byte misalignment (the register kernel reads the
    segment as aligned 16-byte vectors, `shift` 0..3); S shorter than a window or a hop; S an exact multiple of 32 * hop (the last
    block holds one frame)"""
    _check_raw(f"S{S}_hop{hop}", _audio(5, S, S), _lens(S, 5), _fb(), _window("hann", 400), hop)


@pytest.mark.parametrize("hop", [160, 200, 161])
def test_logmel_length_edges(hop):
    S = 40 * hop + 2
    alen = torch.tensor([0, 1, 150, S - 1, S, 2, hop])
    outs = _check_raw(f"lens_hop{hop}", _audio(7, S, hop), alen, _fb(), _window("hann", 400), hop)
    for out in outs:   # an empty row is log(guard) in every cell
        assert (out[0] == out[0, 0, 0]).all()


# ---------------------------------------------------------------------------------------------- pre-emphasis, guard
@pytest.mark.parametrize("hop", [160, 200])
@pytest.mark.parametrize("preemph", [P97, 0.0])
@pytest.mark.parametrize("guard", [GUARD, TINY])
def test_logmel_preemph_and_log_guard(hop, preemph, guard):
    S = 40 * hop + 1
    _check_raw(f"pre{preemph:.2f}_guard{guard:.1e}_hop{hop}", _audio(3, S, 4), _lens(S, 3), _fb(), _window("hann", 400), hop,
               preemph=preemph, guard=guard)


# ---------------------------------------------------------------------------------------------- dither
@pytest.mark.parametrize("hop", [160, 200, 161])
def test_logmel_dither(hop):
    """the noise is a counter-based hash of (seed, sample index): the three kernels see the same noise and agree as they do without
    it (1e-4, tests/test_kernels_gpu.py); a frame that holds no valid sample is bit for bit the dither-off frame, a frame of valid
    samples is not"""
    o = ops()
    S, n_mels, T = 70 * hop + 37, 80, 71
    audio, alen = _audio(3, S, 77).to(dev), torch.tensor([S, S // 3, 1])
    fb, w = _layout(_fb(), "sparse"), _window("hann", 400).to(dev)

    def run_with(dither):
        def run(variant):
            out = torch.full((3, n_mels, T), float("nan"), device=dev)
            o.logmel(audio, alen.to(dev), w, fb, n_mels, hop=hop, preemph=P97, dither=dither, seed=123, out=out)
            torch.cuda.synchronize()
            return out.cpu()
        return _three_kernels(run)

    on, off = run_with(1e-2), run_with(0.0)
    for k in range(3):
        assert torch.isfinite(on[k]).all() and torch.isfinite(off[k]).all()
    e01, e02 = (on[0] - on[1]).abs().max().item(), (on[0] - on[2]).abs().max().item()
    print(f"[frontend] dither_hop{hop}: kernel 0 vs 1 {e01:.3e}, 0 vs 2 {e02:.3e}")
    assert e01 < 1e-4 and e02 < 1e-4, (e01, e02)
    f = torch.arange(T)
    for k in range(3):
        for b in range(3):
            n = int(alen[b])
            untouched = f * hop - 256 >= n                            # the frame's 512 samples all lie beyond the length
            inside = (f * hop - 256 >= 0) & (f * hop + 256 <= n)      # ... all lie inside it
            assert torch.equal(on[k][b][:, untouched], off[k][b][:, untouched]), (k, b)
            if inside.any():
                differ = (on[k][b][:, inside] != off[k][b][:, inside]).float().mean().item()
                assert differ > 0.99, (k, b, differ)
        assert untouched.any() and not inside.any()                   # (the last row: one sample)
    # another seed is another noise
    other = torch.full((3, n_mels, T), float("nan"), device=dev)
    o.logmel(audio, alen.to(dev), w, fb, n_mels, hop=hop, preemph=P97, dither=1e-2, seed=124, out=other)
    torch.cuda.synchronize()
    assert not torch.equal(other.cpu()[0], on[2][0])


# ---------------------------------------------------------------------------------------------- mi355x_feat_normalize
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pad_value", [0.0, -2.5])
def test_feat_normalize_against_float64(normalize, out_dtype, pad_value):
    """35 rows (four per workgroup: the last workgroup holds three), 70 frames (more than one per lane), lengths 0, 1, 2, T"""
    o = ops()
    B, n_mels, T = 5, 7, 70
    g = torch.Generator().manual_seed(3)
    raw = -8.0 + 2.0 * torch.randn(B, n_mels, T, generator=g)
    n = torch.tensor([0, 1, 2, T, 33])
    want = FO.feat_normalize(raw.double(), n, normalize, pad_value)
    out = torch.full((B, n_mels, T), float("nan"), device=dev, dtype=out_dtype)
    o.feat_normalize(raw.to(dev), n.to(dev), out=out, normalize=normalize, pad_value=pad_value, out_dtype=out_dtype)
    torch.cuda.synchronize()
    got = out.cpu()
    assert got.dtype == out_dtype and torch.isfinite(got).all()
    if out_dtype == torch.float32 and not normalize:
        assert torch.equal(got.double(), want)       # a copy and a fill
        return
    tol = (1e-3 if normalize else 0.0) + (2.0 ** -8 * want.abs() if out_dtype == torch.bfloat16 else 0.0)
    err = (got.double() - want).abs()
    print(f"[frontend] feat_normalize normalize={normalize} {out_dtype} pad={pad_value}: max|err| {err.max().item():.3e}")
    assert (err <= tol).all(), err.max().item()
    tmask = torch.arange(T)[None, None, :] >= n[:, None, None]
    assert (got.double()[tmask.expand_as(got)] == float(torch.tensor(pad_value).to(out_dtype))).all()


# ---------------------------------------------------------------------------------------------- the module, end to end
@pytest.mark.parametrize("kw", [dict(window_stride=0.0125), dict(window_size=0.032), dict(features=128),
                                dict(sample_rate=22050, window_size=0.02), dict(normalize="NA"), dict(pad_to=0), dict(pad_to=16),
                                dict(log_zero_guard_value="tiny"),
                                dict(window_stride=0.0125, window_size=0.032, window="hamming", preemph=0.0, pad_value=-4.0)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_preprocessor_module_end_to_end(kw):
    from nemo_amd.modules.audio_preprocessing import AudioToMelSpectrogramPreprocessor
    cfg = dict(sample_rate=16000, window_size=0.025, window_stride=0.01, features=80, dither=0.0, pad_to=16)
    cfg.update(kw)
    m = AudioToMelSpectrogramPreprocessor(**cfg).to(dev).eval()
    f = m.featurizer
    hop, win, sr = f.hop_length, f.win_length, cfg["sample_rate"]
    assert hop == int(cfg["window_stride"] * sr) and win == int(cfg["window_size"] * sr) and f.window.numel() == win
    S = int(1.3 * sr) + 3
    audio = _audio(4, S, 21)
    alen = torch.tensor([S, S // 2, hop, 0])
    feat, n = m(input_signal=audio.to(dev), length=alen.to(dev))
    torch.cuda.synchronize()
    guard = TINY if cfg.get("log_zero_guard_value") == "tiny" else GUARD
    pre = float(np.float32(cfg.get("preemph", 0.97)))
    args = (audio, alen, f.fb[0].cpu(), f.window.cpu(), hop)
    okw = dict(preemph=pre, log_guard=guard, normalize=cfg.get("normalize", "per_feature"),
               pad_value=cfg.get("pad_value", 0.0), pad_to=cfg["pad_to"])
    want, want_n = FO.log_mel_features(*args, **okw)
    assert torch.equal(n.cpu(), want_n) and want_n.tolist() == [S // hop, S // 2 // hop, 1, 0]
    T = 1 + S // hop
    assert feat.shape == want.shape == (4, cfg["features"], (T + 15) // 16 * 16 if cfg["pad_to"] else T)
    assert feat.dtype == torch.float32 and torch.isfinite(feat).all()
    err = (feat.cpu().double() - want).abs().max().item()
    if cfg.get("normalize", "per_feature") == "per_feature":
        tol = 1e-3
    else:
        want32, _ = FO.log_mel_features(*args, dtype=torch.float32, **okw)
        tol = TOL_MULT * (want32.double() - want).abs().max().item()
        assert 0.0 < tol < 1e-2
    print(f"[frontend] module {kw}: max|err| {err:.3e}  tol {tol:.3e}")
    assert err <= tol, (err, tol)


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("what", ["hop>512", "win>512", "T!=1+S//hop", "T one short"])
def test_logmel_refuses_bad_arguments_and_writes_nothing(what):
    from nemo_amd._lib import lib
    o = ops()
    S, hop, win = 4000, 160, 400
    if what == "hop>512":
        hop = 514
    if what == "win>512":
        win = 513
    T = 1 + S // hop + {"T!=1+S//hop": 1, "T one short": -1}.get(what, 0)
    audio, alen = _audio(2, S, 1).to(dev), torch.tensor([S, S]).to(dev)
    w, (st, ln, off, fw) = torch.ones(win, device=dev), _layout(_fb(), "sparse")
    out = torch.full((2, 80, 1 + S // 160 + 2), float("nan"), device=dev)

    def run(variant):
        rc = lib.mi355x_logmel_fwd(o._ptr(audio), o._ptr(alen), o._ptr(w), win, hop, 512, o._ptr(st), o._ptr(ln), o._ptr(off),
                                   o._ptr(fw), 80, P97, 0.0, 0, GUARD, o._ptr(out), 2, S, T, o._stream())
        torch.cuda.synchronize()
        return rc

    assert _three_kernels(run) == [MI_ERR_ARG] * 3
    assert torch.isnan(out).all()
    if what in ("hop>512", "win>512"):   # the wrapper turns the code into the reference's ValueError
        with pytest.raises(ValueError):
            o.logmel(audio, alen, w, (st, ln, off, fw), 80, hop=hop)
