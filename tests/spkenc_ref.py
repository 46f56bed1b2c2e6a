"""Float64 numpy restatement of the speaker encoder (dict_tts_amd/speaker_encoder.py, csrc/spkenc.hip; the specification is in
include/dicttts_hip.h at DTTS_OUT_SPKENC): Resemblyzer 0.1.1's VoiceEncoder — the power mel, the partial slices, the three-layer LSTM,
relu(linear), the norms and the mean over partials.  tests/test_spkenc_cpu.py anchors it on float64 torch (nn.LSTM, torch.stft).

Also the float32 torch forms of the same stages, stage by stage on the CPU: the yardstick of the GPU tests' error gates."""
import numpy as np
import torch

from dict_tts_amd import melspec

SR, N_FFT, HOP, N_MELS, PART, H = 16000, 400, 160, 40, 160, 256


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


def f64(sd):
    return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float64) for k, v in sd.items()}


def lstm_layers(sd, mels):
    """sd float64, mels [N, T, 40] -> every layer's hidden sequence, 3 x [N, T, 256] (gate order i, f, g, o; zero initial state)"""
    x = np.asarray(mels, np.float64)
    out = []
    for k in range(3):
        wih, whh = sd[f"lstm.weight_ih_l{k}"], sd[f"lstm.weight_hh_l{k}"]
        b = sd[f"lstm.bias_ih_l{k}"] + sd[f"lstm.bias_hh_l{k}"]
        N, T = x.shape[0], x.shape[1]
        h, c = np.zeros((N, H)), np.zeros((N, H))
        hs = np.empty((N, T, H))
        for t in range(T):
            g = x[:, t] @ wih.T + h @ whh.T + b
            i, f, gg, o = sigmoid(g[:, :H]), sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), sigmoid(g[:, 3 * H:])
            c = f * c + i * gg
            h = o * np.tanh(c)
            hs[:, t] = h
        out.append(hs)
        x = hs
    return out


def head(sd, h_last):
    """relu(linear(h)) divided by its L2 norm, [N, 256]; a zero row divides to NaN"""
    y = np.maximum(h_last @ sd["linear.weight"].T + sd["linear.bias"], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return y / np.linalg.norm(y, axis=1, keepdims=True)


def forward(sd, mels):
    """-> (unit embeddings [N, 256], the three hidden sequences)"""
    hs = lstm_layers(sd, mels)
    return head(sd, hs[2][:, -1]), hs


def pad_signal(wav, pad_mode):
    wav = np.asarray(wav, np.float64)
    return np.pad(wav, N_FFT // 2, mode="reflect" if pad_mode == "reflect" else "constant")


def mel(wav, pad_mode="constant"):
    """librosa.feature.melspectrogram(wav, 16000, n_fft=400, hop_length=160, n_mels=40).T in float64: [1 + len // 160, 40]"""
    y = pad_signal(wav, pad_mode)
    n = 1 + (len(y) - N_FFT) // HOP
    idx = np.arange(N_FFT)[None, :] + HOP * np.arange(n)[:, None]
    spec = np.fft.rfft(y[idx] * melspec.hann_window(N_FFT)[None, :], axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    return power @ melspec.mel_filterbank(SR, N_FFT, N_MELS, 0, SR // 2).T


def partial_starts(n_samples, rate=1.3, min_coverage=0.75):
    """first frames of the partials of an n_samples utterance (compute_partial_slices)"""
    frame_step = int(np.round((SR / rate) / HOP))
    n_frames = int(np.ceil((n_samples + 1) / HOP))
    steps = max(1, n_frames - PART + frame_step + 1)
    starts = list(range(0, steps, frame_step))
    coverage = (n_samples - starts[-1] * HOP) / (PART * HOP)
    if coverage < min_coverage and len(starts) > 1:
        starts = starts[:-1]
    return starts


def embed_utterance(sd, wav, rate=1.3, min_coverage=0.75, pad_mode="constant", mels=None):
    """-> dict: embed [256], partials [P, 256], mel [F, 40], starts, hseq.  mels: the mel to run the encoder on instead of the float64
    one (the float32 mel of another implementation: the LSTM stage alone)"""
    wav = np.asarray(wav, np.float64).reshape(-1)
    starts = partial_starts(len(wav), rate, min_coverage)
    stop = (starts[-1] + PART) * HOP
    if stop > len(wav):
        wav = np.pad(wav, (0, stop - len(wav)))
    m = mel(wav, pad_mode)
    src = m if mels is None else np.asarray(mels, np.float64)
    parts, hs = forward(sd, np.stack([src[s:s + PART] for s in starts]))
    raw = parts.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"embed": raw / np.linalg.norm(raw), "partials": parts, "mel": m, "starts": starts, "hseq": hs}


# ---- the float32 torch forms (CPU)
def torch_lstm(sd, dtype=torch.float32):
    """(three single-layer nn.LSTM of layer k's weights, nn.Linear): together nn.LSTM(40, 256, 3, batch_first=True), layer by layer"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    layers = []
    for k in range(3):
        m = torch.nn.LSTM(N_MELS if k == 0 else H, H, 1, batch_first=True).to(dtype)
        m.load_state_dict({n: T(sd[f"lstm.{n[:-1]}{k}"]) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
        layers.append(m)
    lin = torch.nn.Linear(H, H).to(dtype)
    lin.load_state_dict({"weight": T(sd["linear.weight"]), "bias": T(sd["linear.bias"])})
    return layers, lin


def torch_forward(sd, mels, dtype=torch.float32):
    """VoiceEncoder.forward in torch at `dtype` -> (unit embeddings [N, 256], the three hidden sequences) as float64 numpy"""
    layers, lin = torch_lstm(sd, dtype)
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(mels)).to(dtype)
        hs = []
        for m in layers:
            x, _ = m(x)
            hs.append(x)
        y = torch.relu(lin(hs[2][:, -1]))
        e = y / torch.norm(y, dim=1, keepdim=True)
    return e.double().numpy(), [h.double().numpy() for h in hs]


def torch_mel(wav, pad_mode="constant", dtype=torch.float32):
    """torch.stft(n_fft 400, hop 160, periodic Hann, center=True) -> power -> the filterbank, at `dtype`: [1 + len // 160, 40]"""
    x = torch.from_numpy(np.ascontiguousarray(wav)).to(dtype)
    win = torch.from_numpy(melspec.hann_window(N_FFT)).to(dtype)
    spec = torch.stft(x, N_FFT, HOP, N_FFT, win, center=True, pad_mode=pad_mode, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2
    fb = torch.from_numpy(melspec.mel_filterbank(SR, N_FFT, N_MELS, 0, SR // 2)).to(dtype)
    return (fb @ power).T.double().numpy()


def torch_embed_utterance(sd, wav, rate=1.3, min_coverage=0.75, pad_mode="constant", dtype=torch.float32):
    """embed_utterance in torch at `dtype`: torch.stft -> nn.LSTM -> the mean in float32 as numpy forms it"""
    wav = np.asarray(wav, np.float32).reshape(-1)
    starts = partial_starts(len(wav), rate, min_coverage)
    stop = (starts[-1] + PART) * HOP
    if stop > len(wav):
        wav = np.pad(wav, (0, stop - len(wav)))
    m = torch_mel(wav, pad_mode, dtype)
    parts, _ = torch_forward(sd, np.stack([m[s:s + PART] for s in starts]), dtype)
    raw = parts.astype(np.float32).mean(axis=0) if dtype == torch.float32 else parts.mean(axis=0)
    return {"embed": (raw / np.linalg.norm(raw, 2)).astype(np.float64), "partials": parts, "mel": m}
