"""float64 numpy restatement of the reference's log-mel front end, data_gen/tts/data_gen_utils.py:122-134 (process_utterance with
vocoder='pwg', loud_norm=False, trim_long_sil=False):

    x_stft = librosa.stft(wav, n_fft, hop_length, win_length, window='hann', pad_mode='constant')     # center=True
    mel = librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) @ np.abs(x_stft)
    mel = np.log10(np.maximum(eps, mel))

librosa is not at hand where this suite is built, so no fixture can come from process_utterance itself; tests/test_melspec_cpu.py
pins this restatement against an independent STFT (torch.stft) and pins the filterbank by its defining properties.

Also here: the SAME pipeline in the reference's own working precision (librosa's STFT of a float32 waveform is a float32 FFT), which
sets the scale of the accuracy bound of tests/test_melspec_gpu.py, and the error figures both are judged by.
"""
import numpy as np

EPS = 1e-6


def hann(win):
    """scipy.signal.get_window('hann', win, fftbins=True)"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)


def frames_of(wav, n_fft, hop, dtype=np.float64):
    """center=True, pad_mode='constant': n_fft // 2 zeros on both sides; frame t = padded[t * hop : t * hop + n_fft]; 1 + len // hop frames"""
    wav = np.asarray(wav, dtype).reshape(-1)
    T = 1 + len(wav) // hop
    pad = np.zeros(len(wav) + n_fft, dtype)
    pad[n_fft // 2:n_fft // 2 + len(wav)] = wav
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    return pad[idx]


def window_of(n_fft, win, dtype=np.float64):
    """the periodic Hann window of win samples, zero padded and centred to n_fft (librosa.util.pad_center: left pad (n_fft - win) // 2)"""
    w = np.zeros(n_fft, np.float64)
    lpad = (n_fft - win) // 2
    w[lpad:lpad + win] = hann(win)
    return w.astype(dtype)


def stft_mag(wav, n_fft, hop, win):
    """|rfft| per frame, float64: [T, n_fft // 2 + 1]"""
    return np.abs(np.fft.rfft(frames_of(wav, n_fft, hop) * window_of(n_fft, win)[None, :], axis=1))


def mel_lin(wav, n_fft, hop, win, mel_basis):
    """mel_basis [n_mels, bins] (any float dtype; librosa's is float32) -> linear mel [T, n_mels], float64"""
    return stft_mag(wav, n_fft, hop, win) @ np.asarray(mel_basis, np.float64).T


def log_mel(lin, eps=EPS):
    return np.log10(np.maximum(eps, lin))


def mel_lin_f32(wav, n_fft, hop, win, mel_basis):
    """the reference's own arithmetic on a float32 waveform: float32 window product, float32 FFT (scipy.fft keeps the input precision, as
    the FFT under librosa.stft does), float32 magnitude, float32 mel product"""
    import scipy.fft
    fr = frames_of(wav, n_fft, hop, np.float32) * window_of(n_fft, win, np.float32)[None, :]
    spec = scipy.fft.rfft(fr, axis=1)
    assert spec.dtype == np.complex64
    return (np.abs(spec) @ np.asarray(mel_basis, np.float32).T).astype(np.float32)


def lin_error(lin, lin64):
    """max |lin - lin64| in units of each frame's largest mel value (floored at 1e-6, the eps of the logarithm)"""
    lin64 = np.asarray(lin64, np.float64)
    scale = np.maximum(lin64.max(axis=1, keepdims=True), 1e-6)
    return float(np.max(np.abs(np.asarray(lin, np.float64) - lin64) / scale))


def log_selection(lin64, rel=1e-3):
    """the entries the log-domain check looks at: mel64 >= rel x the frame's maximum (and above the floor)"""
    lin64 = np.asarray(lin64, np.float64)
    return (lin64 >= rel * lin64.max(axis=1, keepdims=True)) & (lin64 > EPS)


def log_error(logmel, lin64, sel):
    return float(np.max(np.abs(np.asarray(logmel, np.float64) - log_mel(lin64))[sel])) if sel.any() else 0.0


NOISY = ("noise", "clipped", "quiet", "speech")   # the signals that also get the log-domain check


def signals(sr, hop, seed=0):
    """the test signals, float32, 40 * hop + 77 samples each"""
    L = 40 * hop + 77
    rng = np.random.default_rng(seed)
    t = np.arange(L) / sr
    harm = sum(np.sin(2 * np.pi * 140.0 * h * t + 0.7 * h * h) / h for h in range(1, 40))   # 39 harmonics of 140 Hz: up to 5460 Hz
    speech = 0.25 * harm / np.abs(harm).max() * (1.0 + 0.8 * np.sin(2 * np.pi * 3.0 * t)) + 1e-3 * rng.standard_normal(L)
    return {k: np.ascontiguousarray(v, np.float32) for k, v in {
        "noise": 0.1 * rng.standard_normal(L),
        "clipped": np.tanh(2.0 * rng.standard_normal(L)),
        "quiet": 1e-4 * rng.standard_normal(L),
        "speech": speech,
        "tone": 0.9 * np.sin(2 * np.pi * 1000.0 * t),
        "silence": np.zeros(L),
    }.items()}
