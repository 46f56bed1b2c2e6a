"""HifiGAN's discriminators as a measurement on the device: what the reference's vocoder task logs next to ``mel`` —
``a_p`` / ``a_s`` (``generator_loss`` of the MultiPeriodDiscriminator / MultiScaleDiscriminator outputs), ``r_p`` / ``f_p`` / ``r_s`` / ``f_s``
(``discriminator_loss``) and ``fm_f`` / ``fm_s`` (``feature_loss``), modules/hifigan/hifigan.py:154-338 and tasks/vocoder/hifigan.py — computed
by dict_tts_amd/csrc/disc.hip and gconv.hip (dtts_text2mel_fetch(DTTS_OUT_DISC)) from the ``model_disc`` child of a vocoder checkpoint.

Every utterance is scored as if alone at its own length; the library returns fp64 sums and counts, this module forms the per-utterance
figures and the pooled ones (sums over the batch divided by counts over the batch = the reference's batch means when all lengths are
equal).  Gradients, ``use_cond_disc`` and the spectrogram discriminator (``use_spec_disc``) are not implemented and are refused by name.
"""
import numpy as np
import torch

from . import abi
from .unit import DeviceUnit

MPD_CONVS, MSD_CONVS = 5, 7


def fold_weight_norm(g, v, dtype=np.float32):
    """torch.nn.utils.weight_norm(dim=0) folded: w = v * (g / ||v||), the norm over every dimension but the first"""
    g, v = np.asarray(g, dtype), np.asarray(v, dtype)
    n = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1, dtype=dtype)).reshape((-1,) + (1,) * (v.ndim - 1))
    return (v * (g.reshape(n.shape) / n)).astype(dtype)


def fold_spectral_norm(w_orig, u, v, dtype=np.float32):
    """torch.nn.utils.spectral_norm in eval mode (no power iteration): w = weight_orig / (u . (W v)), W = weight_orig as [C_out, -1]"""
    w_orig, u, v = np.asarray(w_orig, dtype), np.asarray(u, dtype), np.asarray(v, dtype)
    sigma = np.dot(u, w_orig.reshape(w_orig.shape[0], -1) @ v)
    return (w_orig / sigma).astype(dtype)


def _layer_names():
    for i in range(len(abi.DISC_PERIODS)):
        for j in range(MPD_CONVS):
            yield f"mpd.discriminators.{i}.convs.{j}", f"mpd.{i}.convs.{j}"
        yield f"mpd.discriminators.{i}.conv_post", f"mpd.{i}.conv_post"
    for i in range(3):
        for j in range(MSD_CONVS):
            yield f"msd.discriminators.{i}.convs.{j}", f"msd.{i}.convs.{j}"
        yield f"msd.discriminators.{i}.conv_post", f"msd.{i}.conv_post"


def fold_state_dict(model_disc, dtype=np.float32):
    """``state_dict.model_disc`` (numpy arrays or tensors) -> the plain weights the library takes: ``mpd.<i>.convs.<j>.{weight,bias}``,
    ``mpd.<i>.conv_post.*``, ``msd.<i>.*``.  A layer comes as ``weight`` (already plain), as ``weight_g`` / ``weight_v`` (weight norm) or as
    ``weight_orig`` / ``weight_u`` / ``weight_v`` (spectral norm, folded in its eval form).  dtype=np.float64 folds the float32 parameters in
    float64, as ``module.double()`` of the reference does (the yardstick of the tests)."""
    np_ = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    sd = {k: np_(v) for k, v in model_disc.items()}
    for k in sd:
        if ".cond_net." in k:
            raise ValueError(f"model_disc holds {k}: a checkpoint trained with use_cond_disc: true; the conditional discriminators are not implemented")
        if k.startswith("specd."):
            raise ValueError(f"model_disc holds {k}: a checkpoint trained with use_spec_disc: true; the spectrogram discriminator is not implemented")
    out = {}
    for src, dst in _layer_names():
        if src + ".weight" in sd:
            w = sd[src + ".weight"].astype(dtype)
        elif src + ".weight_orig" in sd:
            for s in ("weight_u", "weight_v"):
                if f"{src}.{s}" not in sd:
                    raise KeyError(f"model_disc lacks {src}.{s}")
            w = fold_spectral_norm(sd[src + ".weight_orig"], sd[src + ".weight_u"], sd[src + ".weight_v"], dtype)
        elif src + ".weight_g" in sd and src + ".weight_v" in sd:
            w = fold_weight_norm(sd[src + ".weight_g"], sd[src + ".weight_v"], dtype)
        else:
            raise KeyError(f"model_disc lacks {src}.weight (or its weight_g / weight_v, or weight_orig / weight_u / weight_v)")
        if src + ".bias" not in sd:
            raise KeyError(f"model_disc lacks {src}.bias")
        out[dst + ".weight"] = w
        out[dst + ".bias"] = sd[src + ".bias"].astype(dtype)
    return out


def check_hparams(hp):
    """the discriminator options of the vocoder task this module does not implement, refused by name"""
    for key in ("use_cond_disc", "use_spec_disc"):
        if hp and hp.get(key):
            raise ValueError(f"{key}: true is not supported (Discriminators scores MultiPeriodDiscriminator and MultiScaleDiscriminator without conditioning)")


def model_disc_of(path_or_state):
    """a checkpoint path, a loaded checkpoint, its ``state_dict`` or the ``model_disc`` child itself -> the ``model_disc`` child (flat
    keys ``mpd.discriminators...``); KeyError when the checkpoint carries none"""
    st = path_or_state
    if isinstance(st, (str, bytes)) or hasattr(st, "__fspath__"):
        st = torch.load(st, map_location="cpu", weights_only=False)
    if "state_dict" in st:
        st = st["state_dict"]
    if "model_disc" in st:
        return st["model_disc"]
    if any(k.startswith("model_disc.") for k in st):
        return {k[len("model_disc."):]: v for k, v in st.items() if k.startswith("model_disc.")}
    if any(k.startswith(("mpd.", "msd.")) for k in st):
        return st
    raise KeyError("the checkpoint carries no model_disc (only vocoder checkpoints saved by the training task do)")


def figures(sums, counts, fm=None, fm_counts=None):
    """the library's sums -> the reference's figures.  sums f64 [B, 8, 4], counts i64 [B, 8], fm / fm_counts [B, 8, 8] or None (tensors or
    arrays) -> dict: ``a_p, r_p, f_p, a_s, r_s, f_s`` (and ``fm_f, fm_s``) [B] per utterance, and the same names + ``_batch``: sums over the
    batch divided by counts over the batch.  A discriminator that did not run (count 0) gives NaN."""
    T = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    sums, counts = T(sums).to(torch.float64), T(counts).to(torch.float64)
    out = {}
    for tag, sl in (("p", slice(0, 5)), ("s", slice(5, 8))):
        for name, q in (("a", 2), ("r", 0), ("f", 3)):
            out[f"{name}_{tag}"] = (sums[:, sl, q] / counts[:, sl]).mean(dim=1)
            out[f"{name}_{tag}_batch"] = (sums[:, sl, q].sum(0) / counts[:, sl].sum(0)).mean()
    if fm is not None:
        fm, fmc = T(fm).to(torch.float64), T(fm_counts).to(torch.float64)
        for tag, sl, nl in (("f", slice(0, 5), 6), ("s", slice(5, 8), 8)):
            out[f"fm_{tag}"] = 2.0 * (fm[:, sl, :nl] / fmc[:, sl, :nl]).sum(dim=(1, 2))
            out[f"fm_{tag}_batch"] = 2.0 * (fm[:, sl, :nl].sum(0) / fmc[:, sl, :nl].sum(0)).sum()
    return out


class Discriminators(DeviceUnit):
    """``Discriminators(weights)``: plain folded weights (``fold_state_dict``'s names) -> ``scores(y, y_hat, lens)``.

    ctx: an existing ``abi.Context`` (e.g. the vocoder's), or None for one of its own; it is created on the first call, so that argument
    errors surface without a GPU."""

    PREFIX, PART = "disc", abi.PART_DISC

    def __init__(self, weights, ctx=None):
        self.weights = {k: np.ascontiguousarray(np.asarray(v, np.float32)) for k, v in weights.items()}
        self.ctx = ctx

    @classmethod
    def from_checkpoint(cls, path_or_state, hparams=None, ctx=None):
        """a vocoder checkpoint (path, loaded dict, ``state_dict`` or ``model_disc``) -> Discriminators: reads ``state_dict.model_disc``,
        folds weight norm (g v / ||v||) and, for ``msd.discriminators.0``, spectral norm in its eval form.  hparams: the vocoder task's, to
        refuse use_cond_disc / use_spec_disc by name (a ``cond_net`` or ``specd`` key in the checkpoint is refused too)."""
        check_hparams(hparams)
        return cls(fold_state_dict(model_disc_of(path_or_state)), ctx=ctx)

    def scores(self, y, y_hat, lens=None, feature_matching=False, which=("mpd", "msd"), return_d=False):
        """y (recordings), y_hat (generated) [B, T] float32, lens [B] valid samples of both or None (= T) -> dict of float64 device tensors:
        ``a_p, r_p, f_p`` (MPD) and ``a_s, r_s, f_s`` (MSD) [B], with feature_matching=True ``fm_f, fm_s`` [B], each also pooled as
        ``<name>_batch``; the raw ``sums`` [B, 8, 4], ``counts`` [B, 8], ``fm`` / ``fm_counts`` [B, 8, 8] and ``status`` i32 [B]
        (abi.DISC_TOO_SHORT where a device-resident length is outside 6 .. T); return_d=True adds ``d`` f32 [8, 2, B, d_ld]: the D outputs.
        lens given on the host (list, array, CPU tensor) are checked here: a length below abi.DISC_MIN_LEN = 6 samples is refused, as the
        reference's reflect padding refuses it."""
        y, y_hat = torch.as_tensor(y), torch.as_tensor(y_hat)
        if y.dim() != 2 or y.shape != y_hat.shape:
            raise ValueError(f"y and y_hat must both be [B, T] (got {tuple(y.shape)} and {tuple(y_hat.shape)})")
        B, T = y.shape
        if B < 1 or B > 65535:
            raise ValueError(f"B = {B} (supported: 1 .. 65535)")
        if T < abi.DISC_MIN_LEN:
            raise ValueError(f"T = {T} samples is below DISC_MIN_LEN = {abi.DISC_MIN_LEN}, the shortest waveform the reference's discriminators accept")
        bits = 0
        for w in which:
            if w not in ("mpd", "msd"):
                raise ValueError(f"which = {which!r} (any of 'mpd', 'msd')")
            bits |= abi.DISC_MPD if w == "mpd" else abi.DISC_MSD
        if not bits:
            raise ValueError("which is empty: nothing to score")
        if feature_matching:
            bits |= abi.DISC_FM
        if lens is not None:
            lens = torch.as_tensor(lens).reshape(-1)
            if lens.shape[0] != B:
                raise ValueError(f"lens has {lens.shape[0]} entries for a batch of {B}")
            if not lens.is_cuda:
                for b, n in enumerate(lens.tolist()):
                    if n < abi.DISC_MIN_LEN:
                        raise ValueError(f"lens[{b}] = {n} samples is below DISC_MIN_LEN = {abi.DISC_MIN_LEN}, the shortest waveform the "
                                         f"reference's discriminators accept (period 11 pads by reflection)")
                    if n > T:
                        raise ValueError(f"lens[{b}] = {n} samples for waveforms of {T}")
        ctx = self._context()
        dev = self.device
        yd = y.to(device=dev, dtype=torch.float32).contiguous()
        yh = y_hat.to(device=dev, dtype=torch.float32).contiguous()
        ld = None if lens is None else lens.to(device=dev, dtype=torch.int32).contiguous()
        out = {"sums": torch.full((B, 8, 4), float("nan"), dtype=torch.float64, device=dev),
               "counts": torch.zeros((B, 8), dtype=torch.int64, device=dev),
               "status": torch.zeros(B, dtype=torch.int32, device=dev)}
        if feature_matching:
            out["fm"] = torch.full((B, 8, 8), float("nan"), dtype=torch.float64, device=dev)
            out["fm_counts"] = torch.zeros((B, 8, 8), dtype=torch.int64, device=dev)
        d_ld = abi.disc_d_ld(T)
        if return_d:
            out["d"] = torch.full((8, 2, B, d_ld), float("nan"), dtype=torch.float32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        ctx.disc(B, torch.cuda.current_stream().cuda_stream, y=yd.data_ptr(), y_hat=yh.data_ptr(), wav_ld=T, which=bits, lens=ptr(ld),
                 sums=out["sums"].data_ptr(), counts=out["counts"].data_ptr(), status=out["status"].data_ptr(), fm=ptr(out.get("fm")),
                 fm_counts=ptr(out.get("fm_counts")), d=ptr(out.get("d")), d_ld=d_ld if return_d else 0)
        out.update(figures(out["sums"], out["counts"], out.get("fm"), out.get("fm_counts")))
        return out
