"""ctypes binding of libdicttts_hip.so (include/dicttts_hip.h).  No torch types cross the boundary: device
pointers are passed as integers (``tensor.data_ptr()``), the stream as ``torch.cuda.current_stream().cuda_stream``.

There is NO CPU fallback here: if the shared library is missing, or no GPU is visible, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdicttts_hip.so")

DTTS_F32, DTTS_I64 = 0, 1
VOC_BF16, VOC_BF16X3, VOC_F16 = 0, 1, 2
VOC_PRECISIONS = {"f16": VOC_F16, "bf16": VOC_BF16, "bf16x3": VOC_BF16X3}
PART_ACOUSTIC, PART_VOCODER, PART_FFT = 1, 2, 4
PART_MELSPEC = 8    # the log-mel front end: "melspec.mel_basis" + "melspec.window"; rebuilt by every finalize that names it
PART_STFT = 16      # the multi-resolution STFT distance: "stft.<i>.window" [n_fft], up to four; rebuilt by every finalize that names it
PART_ISTFT = 32     # STFT -> magnitude edit -> inverse STFT: "istft.window" [n_fft]; rebuilt by every finalize that names it
OUT_PRON_ATTN, OUT_DUR, OUT_MEL2WORD, OUT_DICT_ATTN, OUT_WORD_ENCODER_OUT, OUT_X_MASK, OUT_CONTEXT, OUT_MEL_LENS = range(1, 9)
OUT_POSTERIOR = 9   # not a copy: the posterior pass, dst = a PosteriorArgs block (include/dicttts_hip.h)
OUT_MELSPEC = 10     # not a copy, needs no encode: wav -> log-mel, dst = a MelspecArgs block
OUT_STFT_DISTANCE = 11   # not a copy, needs no encode: a pair of waveform batches -> the sums behind sc / mag, dst = a StftArgs block
OUT_SPECTRAL = 12    # not a copy, needs no encode: STFT / edit / inverse STFT of a batch of waveforms, dst = a SpectralArgs block
OUT_GRIFFIN_LIM = 13   # not a copy, needs no encode: magnitudes (or log10-mels) -> waveforms by Griffin-Lim, dst = a GriffinLimArgs block
OUT_LOSSES = 14   # not a copy, needs no encode: the sums behind validation_step's mel (l1 / mse / ssim) and word-duration losses, dst = a LossArgs block
LOSS_TILE_ROWS = 32   # DTTS_LOSS_TILE_ROWS: frames per tile of the mel half (the shape cases of tests/losses_shapes.py derive from it)
LOSS_MAX_WORDS = 16384   # DTTS_LOSS_MAX_WORDS
OUT_DTW = 15   # not a copy, needs no encode: dynamic time warping of a batch of sequence pairs (distance, path, F0 moments), dst = a DtwArgs block
DTW_STRIP_ROWS = 1024   # DTTS_DTW_STRIP_ROWS: rows one pass of the wave covers (the shape cases of tests/dtw_shapes.py derive from it)
DTW_LANE_ROWS = 16      # rows of a strip one lane owns (DTW_STRIP_ROWS / 64)
DTW_MAX_LEN = 8192      # DTTS_DTW_MAX_LEN
OUT_PITCH = 16   # not a copy, needs no encode: F0 tracks of a batch of waveforms (Praat's autocorrelation method), dst = a PitchArgs block
PITCH_CANDIDATES = 15     # DTTS_PITCH_CANDIDATES
PITCH_MAX_WINDOW = 2048   # DTTS_PITCH_MAX_WINDOW
PITCH_MAX_FRAMES = 8192   # DTTS_PITCH_MAX_FRAMES
DTTS_F64 = 2          # dtts_load_weight takes it for the "resample." tensors only
PART_RESAMPLE = 64    # the band-limited resampler: "resample.filter" [n_win] f64 + "resample.num_table" [1] f64; rebuilt by every finalize that names it
OUT_RESAMPLE = 17     # not a copy, needs no encode: resampy's kaiser-windowed sinc interpolation of a batch of waveforms, dst = a ResampleArgs block
RESAMPLE_TILE = 256   # DTTS_RESAMPLE_TILE: consecutive outputs of one workgroup (the shape cases of tests/wavprep_shapes.py derive from it)
OUT_LOUDNESS = 18     # not a copy, needs no encode or weights: BS.1770 integrated loudness and normalisation, dst = a LoudnessArgs block
LOUD_SEGMENT = 256    # DTTS_LOUD_SEGMENT: samples of one segment of the K-weighting recurrence
LOUD_TOO_SHORT, LOUD_SILENT, LOUD_PEAK = 1, 2, 4   # dtts_loudness_args status bits
PART_DISC = 128       # HifiGAN's discriminators: "disc.mpd.<i>.*" / "disc.msd.<i>.*", plain (folded) weights; built once per context
OUT_DISC = 19         # not a copy, needs no encode: the sums behind a_p / a_s, r_* / f_*, fm_* of a batch of waveform pairs, dst = a DiscArgs block
DISC_MPD, DISC_MSD, DISC_FM = 1, 2, 4   # dtts_disc_args.which bits
DISC_DENSE_GROUPED = 8   # DTTS_DISC_DENSE_GROUPED: measurement aid, the grouped layers as block-diagonal dense layers
DISC_N = 8            # DTTS_DISC_N: discriminators (5 periods, then 3 scales)
DISC_MAX_FMAPS = 8    # DTTS_DISC_MAX_FMAPS
DISC_MIN_LEN = 6      # DTTS_DISC_MIN_LEN: the shortest waveform the reference's discriminators accept
DISC_TOO_SHORT = 1    # DTTS_DISC_TOO_SHORT (status bit)
DISC_DENSE_TILE, DISC_GROUP_TILE, DISC_GROUP_TILE_WIDE = 32, 128, 64   # DTTS_DISC_*_TILE (the shape cases of tests/disc_shapes.py derive from them)
DISC_PERIODS = (2, 3, 5, 7, 11)
PART_SPKENC = 256     # the d-vector speaker encoder: "spkenc.<VoiceEncoder state-dict key>", "spkenc.mel_basis", "spkenc.window"; built once per context
OUT_SPKENC = 20       # not a copy, needs no encode: utterance embeddings of a batch of recordings (or of mel sequences), dst = a SpkencArgs block
SPKENC_FROM_WAV, SPKENC_FROM_MELS = 0, 1             # dtts_spkenc_args.mode
SPKENC_PAD_CONSTANT, SPKENC_PAD_REFLECT = 0, 1       # dtts_spkenc_args.pad_mode
SPKENC_TILE_M = 32    # DTTS_SPKENC_TILE_M: the most sequences per workgroup of the recurrent kernel (tile_m = 16 is the other form)
SPKENC_MAX_T = 4096   # DTTS_SPKENC_MAX_T
SPKENC_HOP, SPKENC_PART, SPKENC_MELS, SPKENC_DIM = 160, 160, 40, 256
PART_MELDISC = 512    # the acoustic checkpoint's multi-window mel discriminator: "meldisc.<w>.*", plain (folded) weights; built once per context
OUT_MELDISC = 21      # not a copy, needs no encode: D per clip and the sums behind a / r / f of a batch of mels, dst = a MeldiscArgs block
MELDISC_STACK, MELDISC_SUM, MELDISC_NONE = 0, 1, 2   # dtts_meldisc_args.reduction
MELDISC_REDUCTIONS = {"stack": MELDISC_STACK, "sum": MELDISC_SUM, "none": MELDISC_NONE}
MELDISC_WITHIN_LEN = 1   # DTTS_MELDISC_WITHIN_LEN (flags): a slot is a clip only where it ends within the signal's own length
MELDISC_BAD_LEN = 1      # DTTS_MELDISC_BAD_LEN (status bit)
MELDISC_MELS, MELDISC_MAX_WIN, MELDISC_D_LD, MELDISC_MAX_HIDDEN = 80, 3, 16, 256
MELDISC_WINS = (32, 64, 128)
PART_GLOSS = 1024     # the gloss encoder (RoFormer): "gloss.<HF key without 'roformer.'>" + "gloss.config"; built once per context
GLOSS_ENCODE = 64     # DTTS_GLOSS_ENCODE: what dtts_text2mel_fetch takes for a GlossArgs block (not an OUT_ item: it is no output of the text-to-mel path)
GLOSS_MAX_L = 64      # DTTS_GLOSS_MAX_L: tokens per gloss, [CLS] and [SEP] included
PART_PORTASPEECH = 2048   # the PortaSpeech baseline: "ps.<state-dict key>" + "ps.config" + "ps.word_encoder.pos_table"; built once; excludes PART_ACOUSTIC
PS_ENCODE = 65            # DTTS_PS_ENCODE: what dtts_text2mel_fetch takes for a PsArgs block (the baseline's encode; not an OUT_ item)
PS_PH_ENCODER_OUT, PS_ATTN, PS_DECODER_INP = 66, 67, 68   # DTTS_PS_*: the copy items after a PS_ENCODE
PS_BAD_TOKEN, PS_ZERO_TOKEN, PS_BAD_PH2WORD, PS_EMPTY_WORD, PS_BAD_MEL2WORD = 1, 2, 3, 4, 5   # dtts_ps_args status codes
PS_STATUS_NAMES = {PS_BAD_TOKEN: "DTTS_PS_BAD_TOKEN: a token outside [0, n_phone)",
                   PS_ZERO_TOKEN: "DTTS_PS_ZERO_TOKEN: a zero token inside the live prefix",
                   PS_BAD_PH2WORD: "DTTS_PS_BAD_PH2WORD: ph2word must start at 0 or 1, grow by 0 or 1 per live phoneme up to T_w, and be 0 past the live prefix",
                   PS_EMPTY_WORD: "DTTS_PS_EMPTY_WORD: a live frame whose word has no phonemes",
                   PS_BAD_MEL2WORD: "DTTS_PS_BAD_MEL2WORD: mel2word must lie in [0, T_w], be non-decreasing over its non-zero prefix and 0 behind it"}
DICT_EDIT, DICT_ENTRY = 69, 70   # DTTS_DICT_EDIT / DTTS_DICT_ENTRY: replace / append entries of the resident table, read one back (not OUT_ items)
MAX_SENSES = 15                  # DTTS_MAX_SENSES
SPECTRAL_FORWARD, SPECTRAL_INVERSE = 1, 2  # dtts_spectral_args.mode bits; both = the reference's denoise
SPK_EMBED, SPK_ID = 1, 2   # dtts_text2mel_speakers kinds: fp32 [B,256] (use_spk_embed) / int64 [B] (use_spk_id)
TIMER_VOC_CONV, TIMER_S2PA = 1, 2
TIMER_STAGE_ENCODER, TIMER_STAGE_DICT_ENCODER, TIMER_STAGE_FVAE, TIMER_STAGE_HIFIGAN = 3, 4, 5, 6   # the reference's profile_infer names
TIMER_DICT_SEG_COPY = 7   # DTTS_TIMER_DICT_SEG_COPY: the K array's segment-copy launch of every DICT_EDIT

OUT_NAMES = {v: "DTTS_" + k for k, v in list(globals().items()) if k.startswith("OUT_")}   # code -> "DTTS_OUT_X", as the library's messages spell it

EXPORTS = ["dtts_default_config", "dtts_config_sizeof", "dtts_create", "dtts_destroy", "dtts_last_error", "dtts_load_weight",
           "dtts_finalize_weights", "dtts_dict_table_upload", "dtts_text2mel_encode", "dtts_text2mel_encode_ids", "dtts_text2mel_speakers", "dtts_text2mel_decode", "dtts_text2mel_fetch",
           "dtts_load_weights", "dtts_text2mel_plan", "dtts_text2mel_forward", "dtts_text2mel_forward_ids",
           "dtts_length_regulate", "dtts_hifigan_forward", "dtts_hifigan_hop", "dtts_wav_to_int16", "dtts_fft_blocks_forward",
           "dtts_timer_enable", "dtts_timer_read", "dtts_timer_reset", "dtts_set_noise_seed", "dtts_vocoder_range_guard", "dtts_vocoder_clamped", "dtts_vocoder_nonfinite", "dtts_vocoder_fp16_bound",
           "dtts_debug_check", "dtts_debug_poke"]


class PosteriorArgs(C.Structure):
    """dtts_posterior_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_POSTERIOR)"""
    _fields_ = [("size", C.c_int32), ("mel_ld", C.c_int32), ("eps_ld", C.c_int32), ("mel_cap", C.c_int32),
                ("tgt_mels_dev", C.c_void_p), ("eps_dev", C.c_void_p), ("mel_out_dev", C.c_void_p), ("m_q_dev", C.c_void_p),
                ("logs_q_dev", C.c_void_p), ("z_p_dev", C.c_void_p), ("kl_dev", C.c_void_p)]


class MelspecArgs(C.Structure):
    """dtts_melspec_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_MELSPEC)"""
    _fields_ = [("size", C.c_int32), ("hop", C.c_int32), ("B", C.c_int32), ("wav_ld", C.c_int32), ("mel_cap", C.c_int32), ("eps", C.c_float),
                ("wav_dev", C.c_void_p), ("wav_lens_dev", C.c_void_p), ("mel_dev", C.c_void_p), ("mel_lens_dev", C.c_void_p), ("lin_dev", C.c_void_p)]


class StftArgs(C.Structure):
    """dtts_stft_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_STFT_DISTANCE)"""
    _fields_ = [("size", C.c_int32), ("n_res", C.c_int32), ("hop", C.c_int32 * 4), ("B", C.c_int32), ("wav_ld", C.c_int32), ("mag_cap", C.c_int32),
                ("reserved", C.c_int32), ("x_dev", C.c_void_p), ("y_dev", C.c_void_p), ("lens_dev", C.c_void_p), ("sums_dev", C.c_void_p),
                ("count_dev", C.c_void_p), ("mag_dev", C.c_void_p)]


class SpectralArgs(C.Structure):
    """dtts_spectral_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_SPECTRAL)"""
    _fields_ = [("size", C.c_int32), ("mode", C.c_int32), ("hop", C.c_int32), ("B", C.c_int32), ("wav_ld", C.c_int32), ("spec_cap", C.c_int32),
                ("floor", C.c_float), ("wav_dev", C.c_void_p), ("lens_dev", C.c_void_p), ("frames_dev", C.c_void_p), ("spec_dev", C.c_void_p),
                ("out_dev", C.c_void_p), ("out_lens_dev", C.c_void_p)]


class GriffinLimArgs(C.Structure):
    """dtts_griffinlim_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_GRIFFIN_LIM)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("spec_cap", C.c_int32), ("hop", C.c_int32), ("n_iter", C.c_int32), ("wav_ld", C.c_int32),
                ("n_mels", C.c_int32), ("reserved", C.c_int32), ("mag_dev", C.c_void_p), ("mel_dev", C.c_void_p), ("init_dev", C.c_void_p),
                ("frames_dev", C.c_void_p), ("out_dev", C.c_void_p), ("out_lens_dev", C.c_void_p), ("spec_out_dev", C.c_void_p)]


class LossArgs(C.Structure):
    """dtts_loss_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_LOSSES)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("T", C.c_int32), ("n_mel", C.c_int32), ("pred_ld", C.c_int32), ("tgt_ld", C.c_int32),
                ("bias", C.c_float), ("T_w", C.c_int32), ("T_mel", C.c_int32), ("m2w_ld", C.c_int32), ("dur_scale", C.c_int32), ("reserved", C.c_int32),
                ("pred_dev", C.c_void_p), ("tgt_dev", C.c_void_p), ("mel_sums_dev", C.c_void_p), ("mel_count_dev", C.c_void_p),
                ("ssim_map_dev", C.c_void_p), ("dur_pred_dev", C.c_void_p), ("mel2word_dev", C.c_void_p), ("word_len_dev", C.c_void_p),
                ("dur_sums_dev", C.c_void_p), ("dur_gt_dev", C.c_void_p)]


class DtwArgs(C.Structure):
    """dtts_dtw_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_DTW)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("F", C.c_int32), ("dtype", C.c_int32), ("x_ld", C.c_int32), ("y_ld", C.c_int32),
                ("window", C.c_int32), ("path_ld", C.c_int32), ("slope", C.c_double), ("x_dev", C.c_void_p), ("y_dev", C.c_void_p),
                ("x_lens_dev", C.c_void_p), ("y_lens_dev", C.c_void_p), ("dist_dev", C.c_void_p), ("path_dev", C.c_void_p),
                ("path_len_dev", C.c_void_p), ("acc_dev", C.c_void_p), ("moments_dev", C.c_void_p)]


def dtw_args(B, x, y, x_ld, y_ld, dist, F=1, dtype=0, window=-1, slope=1.0, x_lens=None, y_lens=None, path=None, path_ld=0, path_len=None,
             acc=None, moments=None):
    """a filled DtwArgs block (device pointers as integers, 0 / None = NULL)"""
    return DtwArgs(C.sizeof(DtwArgs), int(B), int(F), int(dtype), int(x_ld), int(y_ld), int(window), int(path_ld), float(slope), x or None,
                   y or None, x_lens or None, y_lens or None, dist or None, path or None, path_len or None, acc or None, moments or None)


class PitchArgs(C.Structure):
    """dtts_pitch_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_PITCH)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("wav_ld", C.c_int32), ("frames_ld", C.c_int32), ("sample_rate", C.c_int32), ("hop", C.c_int32),
                ("pitch_floor", C.c_double), ("pitch_ceiling", C.c_double), ("voicing_threshold", C.c_double), ("silence_threshold", C.c_double),
                ("octave_cost", C.c_double), ("octave_jump_cost", C.c_double), ("voiced_unvoiced_cost", C.c_double),
                ("wav_dev", C.c_void_p), ("lens_dev", C.c_void_p), ("f0_dev", C.c_void_p), ("n_frames_dev", C.c_void_p), ("acf_dev", C.c_void_p),
                ("cand_dev", C.c_void_p), ("n_cand_dev", C.c_void_p), ("intensity_dev", C.c_void_p), ("selected_dev", C.c_void_p)]


def pitch_args(B, wav, wav_ld, frames_ld, f0, n_frames, sample_rate=22050, hop=256, pitch_floor=80.0, pitch_ceiling=750.0, voicing_threshold=0.6,
               silence_threshold=0.03, octave_cost=0.01, octave_jump_cost=0.35, voiced_unvoiced_cost=0.14, lens=None, acf=None, cand=None,
               n_cand=None, intensity=None, selected=None):
    """a filled PitchArgs block (device pointers as integers, 0 / None = NULL; the defaults are the reference's and Praat's)"""
    return PitchArgs(C.sizeof(PitchArgs), int(B), int(wav_ld), int(frames_ld), int(sample_rate), int(hop), float(pitch_floor), float(pitch_ceiling),
                     float(voicing_threshold), float(silence_threshold), float(octave_cost), float(octave_jump_cost), float(voiced_unvoiced_cost),
                     wav or None, lens or None, f0 or None, n_frames or None, acf or None, cand or None, n_cand or None, intensity or None,
                     selected or None)


class ResampleArgs(C.Structure):
    """dtts_resample_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_RESAMPLE)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("wav_ld", C.c_int32), ("out_ld", C.c_int32), ("sr_in", C.c_int32), ("sr_out", C.c_int32),
                ("wav_dev", C.c_void_p), ("lens_dev", C.c_void_p), ("out_dev", C.c_void_p), ("out_lens_dev", C.c_void_p), ("out64_dev", C.c_void_p)]


def resample_args(B, wav, wav_ld, out, out_ld, out_lens, sr_in, sr_out, lens=None, out64=None):
    """a filled ResampleArgs block (device pointers as integers, 0 / None = NULL)"""
    return ResampleArgs(C.sizeof(ResampleArgs), int(B), int(wav_ld), int(out_ld), int(sr_in), int(sr_out), wav or None, lens or None, out or None,
                        out_lens or None, out64 or None)


def resample_filter_key(half_window, num_table):
    """what identifies a resampling filter: (n_win, num_table, hash of the table's bytes)"""
    a = np.ascontiguousarray(np.asarray(half_window, np.float64).reshape(-1))
    return (a.shape[0], int(num_table), hash(a.tobytes()))


class LoudnessArgs(C.Structure):
    """dtts_loudness_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_LOUDNESS)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("wav_ld", C.c_int32), ("blocks_ld", C.c_int32), ("sample_rate", C.c_int32), ("mode", C.c_int32),
                ("target_lufs", C.c_double), ("wav_dev", C.c_void_p), ("lens_dev", C.c_void_p), ("lufs_dev", C.c_void_p), ("gain_dev", C.c_void_p),
                ("status_dev", C.c_void_p), ("out_dev", C.c_void_p), ("z_dev", C.c_void_p), ("n_blocks_dev", C.c_void_p)]


def loudness_args(B, wav, wav_ld, blocks_ld, sample_rate, lufs, gain, status, mode=0, target_lufs=-22.0, lens=None, out=None, z=None, n_blocks=None):
    """a filled LoudnessArgs block (device pointers as integers, 0 / None = NULL; -22 LUFS is the reference's loud_norm target)"""
    return LoudnessArgs(C.sizeof(LoudnessArgs), int(B), int(wav_ld), int(blocks_ld), int(sample_rate), int(mode), float(target_lufs), wav or None,
                        lens or None, lufs or None, gain or None, status or None, out or None, z or None, n_blocks or None)


class DiscArgs(C.Structure):
    """dtts_disc_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_DISC)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("wav_ld", C.c_int32), ("which", C.c_int32), ("d_ld", C.c_int32), ("reserved", C.c_int32),
                ("y_dev", C.c_void_p), ("y_hat_dev", C.c_void_p), ("lens_dev", C.c_void_p), ("sums_dev", C.c_void_p), ("counts_dev", C.c_void_p),
                ("fm_dev", C.c_void_p), ("fm_counts_dev", C.c_void_p), ("d_dev", C.c_void_p), ("status_dev", C.c_void_p)]


def disc_d_ld(wav_ld):
    """entries per row of d_dev that dtts_disc_args asks for at wav_ld samples"""
    return (int(wav_ld) + 63) // 64 + 16


def disc_args(B, y, y_hat, wav_ld, sums, counts, status, which=DISC_MPD | DISC_MSD, lens=None, fm=None, fm_counts=None, d=None, d_ld=0):
    """a filled DiscArgs block (device pointers as integers, 0 / None = NULL)"""
    return DiscArgs(C.sizeof(DiscArgs), int(B), int(wav_ld), int(which), int(d_ld), 0, y or None, y_hat or None, lens or None, sums or None,
                    counts or None, fm or None, fm_counts or None, d or None, status or None)


class SpkencArgs(C.Structure):
    """dtts_spkenc_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_SPKENC)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("wav_ld", C.c_int32), ("mode", C.c_int32), ("frame_step", C.c_int32), ("pad_mode", C.c_int32),
                ("tile_m", C.c_int32), ("reserved", C.c_int32), ("min_coverage", C.c_double), ("wav_dev", C.c_void_p), ("lens_dev", C.c_void_p),
                ("embed_dev", C.c_void_p), ("n_partials_dev", C.c_void_p), ("partials_dev", C.c_void_p), ("mel_dev", C.c_void_p),
                ("hseq_dev", C.c_void_p * 3)]


def spkenc_max_partials(wav_ld, frame_step):
    """dtts_spkenc_max_partials: partials of a wav_ld-sample utterance before the coverage rule = rows per utterance of partials / hseq"""
    steps = max(1, (int(wav_ld) // SPKENC_HOP + 1) - SPKENC_PART + int(frame_step) + 1)
    return (steps - 1) // int(frame_step) + 1


def spkenc_frames_ld(wav_ld, frame_step):
    """dtts_spkenc_frames_ld: mel frames per utterance of mel_dev at wav_ld samples"""
    stop = SPKENC_HOP * ((spkenc_max_partials(wav_ld, frame_step) - 1) * int(frame_step) + SPKENC_PART)
    return 1 + max(int(wav_ld), stop) // SPKENC_HOP


def spkenc_args(B, wav, wav_ld, embed, n_partials, mode=SPKENC_FROM_WAV, frame_step=77, min_coverage=0.75, pad_mode=SPKENC_PAD_CONSTANT, tile_m=0,
                lens=None, partials=None, mel=None, hseq=(None, None, None)):
    """a filled SpkencArgs block (device pointers as integers, 0 / None = NULL)"""
    return SpkencArgs(C.sizeof(SpkencArgs), int(B), int(wav_ld), int(mode), int(frame_step), int(pad_mode), int(tile_m), 0, float(min_coverage),
                      wav or None, lens or None, embed or None, n_partials or None, partials or None, mel or None,
                      (C.c_void_p * 3)(*[v or None for v in hseq]))


class MeldiscArgs(C.Structure):
    """dtts_meldisc_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_OUT_MELDISC)"""
    _fields_ = [("size", C.c_int32), ("n_sig", C.c_int32), ("T_ld", C.c_int32), ("n_win", C.c_int32), ("reduction", C.c_int32), ("flags", C.c_int32),
                ("clips_ld", C.c_int32), ("hop", C.c_int32 * 3), ("reserved", C.c_int32 * 2), ("mel_dev", C.c_void_p), ("lens_dev", C.c_void_p),
                ("starts_dev", C.c_void_p), ("d_dev", C.c_void_p), ("sums_dev", C.c_void_p), ("counts_dev", C.c_void_p), ("status_dev", C.c_void_p),
                ("h_dev", C.c_void_p * 9)]


def meldisc_args(n_sig, mel, T_ld, n_win, clips_ld, sums, counts, status, reduction=MELDISC_STACK, flags=0, hop=(0, 0, 0), lens=None, starts=None,
                 d=None, h=(None,) * 9):
    """a filled MeldiscArgs block (device pointers as integers, 0 / None = NULL)"""
    return MeldiscArgs(C.sizeof(MeldiscArgs), int(n_sig), int(T_ld), int(n_win), int(reduction), int(flags), int(clips_ld),
                       (C.c_int32 * 3)(*[int(v) for v in hop]), (C.c_int32 * 2)(0, 0), mel or None, lens or None, starts or None, d or None, sums or None,
                       counts or None, status or None, (C.c_void_p * 9)(*[v or None for v in h]))


class GlossArgs(C.Structure):
    """dtts_gloss_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_GLOSS_ENCODE)"""
    _fields_ = [("size", C.c_int32), ("n_gloss", C.c_int32), ("sum_L", C.c_int32), ("L_max", C.c_int32), ("ids_dev", C.c_void_p),
                ("tok_off_dev", C.c_void_p), ("out_dev", C.c_void_p), ("status_dev", C.c_void_p)]


def gloss_args(n_gloss, ids, tok_off, sum_L, L_max, out, status):
    """a filled GlossArgs block (device pointers as integers, 0 / None = NULL)"""
    return GlossArgs(C.sizeof(GlossArgs), int(n_gloss), int(sum_L), int(L_max), ids or None, tok_off or None, out or None, status or None)


class PsArgs(C.Structure):
    """dtts_ps_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_PS_ENCODE)"""
    _fields_ = [("size", C.c_int32), ("B", C.c_int32), ("T_ph", C.c_int32), ("T_w", C.c_int32), ("T_m2w", C.c_int32), ("want_attn", C.c_int32),
                ("txt_tokens_dev", C.c_void_p), ("ph2word_dev", C.c_void_p), ("mel2word_dev", C.c_void_p), ("status_dev", C.c_void_p),
                ("T_mel_host", C.POINTER(C.c_int32))]


def ps_args(B, T_ph, T_w, txt_tokens, ph2word, status, T_mel, mel2word=None, T_m2w=0, want_attn=True):
    """a filled PsArgs block (device pointers as integers, 0 / None = NULL; T_mel: a ctypes.c_int32 the call writes)"""
    return PsArgs(C.sizeof(PsArgs), int(B), int(T_ph), int(T_w), int(T_m2w), int(bool(want_attn)), txt_tokens or None, ph2word or None,
                  mel2word or None, status or None, C.pointer(T_mel) if T_mel is not None else None)


class DictEditArgs(C.Structure):
    """dtts_dict_edit_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_DICT_EDIT)"""
    _fields_ = [("size", C.c_int32), ("n_edit", C.c_int32), ("rows_on_device", C.c_int32), ("reserved", C.c_int32),
                ("entry_id_host", C.c_void_p), ("tok_off_host", C.c_void_p), ("pin_off_host", C.c_void_p), ("key_map_host", C.c_void_p),
                ("pinyin_host", C.c_void_p), ("pinyin_map_host", C.c_void_p), ("keys", C.c_void_p), ("values", C.c_void_p)]


def dict_edit_args(n_edit, entry_id, tok_off, pin_off, key_map, pinyin, pinyin_map, keys, values=None, rows_on_device=False):
    """a filled DictEditArgs block (pointers as integers, 0 / None = NULL; keys / values are device pointers iff rows_on_device)"""
    return DictEditArgs(C.sizeof(DictEditArgs), int(n_edit), int(bool(rows_on_device)), 0, entry_id or None, tok_off or None, pin_off or None,
                        key_map or None, pinyin or None, pinyin_map or None, keys or None, values or None)


class DictEntryArgs(C.Structure):
    """dtts_dict_entry_args (include/dicttts_hip.h): the argument block of dtts_text2mel_fetch(DTTS_DICT_ENTRY); n_entries, L_e, P_e are written"""
    _fields_ = [("size", C.c_int32), ("entry", C.c_int32), ("n_entries", C.c_int32), ("L_e", C.c_int32), ("P_e", C.c_int32), ("reserved", C.c_int32),
                ("k_dev", C.c_void_p), ("v_dev", C.c_void_p), ("key_map_dev", C.c_void_p), ("pinyin_dev", C.c_void_p), ("pinyin_map_dev", C.c_void_p)]


def dict_entry_args(entry, k=None, v=None, key_map=None, pinyin=None, pinyin_map=None):
    """a filled DictEntryArgs block (device pointers as integers, 0 / None = NULL)"""
    return DictEntryArgs(C.sizeof(DictEntryArgs), int(entry), 0, 0, 0, 0, k or None, v or None, key_map or None, pinyin or None, pinyin_map or None)


class DttsConfig(C.Structure):
    """struct dtts_config (include/dicttts_hip.h); field <- reference hparams key.
    resblock_dilation_sizes: one row per kernel size; three dilations >= 1 = ResBlock1, a row whose third entry is 0 = a two-dilation
    (ResBlock2, ``resblock: "2"``) row; all used rows of one kind (hparams.fill_abi_config writes them from the generator config)."""
    _fields_ = [(n, C.c_int32) for n in (
        "hidden_size", "num_heads", "enc_ffn_kernel_size", "enc_layers", "gloss_dim", "word_size",
        "value_embedding_size", "n_phone", "audio_num_mel_bins", "latent_size", "fvae_enc_dec_hidden",
        "fvae_kernel_size", "fvae_dec_n_layers", "fvae_enc_n_layers", "prior_glow_hidden", "glow_kernel_size",
        "prior_glow_n_blocks", "prior_glow_n_layers", "dur_predictor_layers", "dur_predictor_kernel", "dur_chans",
        "frames_multiple", "language_zh", "upsample_initial_channel", "n_upsamples")] + [
        ("upsample_rates", C.c_int32 * 8), ("upsample_kernel_sizes", C.c_int32 * 8), ("n_resblock_kernels", C.c_int32),
        ("resblock_kernel_sizes", C.c_int32 * 4), ("resblock_dilation_sizes", (C.c_int32 * 3) * 4),
        ("vocoder_precision", C.c_int32), ("fft_layers", C.c_int32), ("fft_kernel_size", C.c_int32),
        ("fft_use_pos_embed", C.c_int32), ("fft_use_last_norm", C.c_int32), ("vocoder_unfused", C.c_int32), ("decoder_fp32", C.c_int32),
        ("vocoder_range_guard", C.c_int32), ("debug_redzone", C.c_int32), ("tune_flags", C.c_int32)]


class DttsError(RuntimeError):
    pass


def ps_status_error(status):
    """None for a clean status word of a PS_ENCODE ([4] integers), else the message naming utterance, code, value and position"""
    st = [int(v) for v in status]
    if st[0] == 0:
        return None
    return f"utterance {st[0] - 1}, position {st[3]}, value {st[2]}: {PS_STATUS_NAMES.get(st[1], f'code {st[1]}')}"


_lib = None


def load_library(path=None):
    """dlopen the in-tree library; raise (never fall back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    try:   # PyTorch-ROCm bundles its own HIP runtime: load it FIRST so that this library binds to the same one (a process that loads
        import torch  # noqa: F401  # the system libamdhip64 first and torch's afterwards ends up with two runtimes and no visible device)
    except ImportError:
        pass
    if not os.path.exists(path):
        raise DttsError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"or `make -C dict_tts_amd/csrc` (there is no CPU fallback for the HIP path)")
    lib = C.CDLL(path)
    vp, i32, i64p = C.c_void_p, C.c_int, C.POINTER(C.c_int64)
    lib.dtts_default_config.argtypes = [C.POINTER(DttsConfig)]
    lib.dtts_default_config.restype = None
    lib.dtts_config_sizeof.argtypes = []
    lib.dtts_config_sizeof.restype = C.c_int
    lib.dtts_create.argtypes = [C.POINTER(DttsConfig), C.POINTER(vp)]
    lib.dtts_destroy.argtypes = [vp]
    lib.dtts_destroy.restype = None
    lib.dtts_last_error.argtypes = [vp]
    lib.dtts_last_error.restype = C.c_char_p
    lib.dtts_load_weight.argtypes = [vp, C.c_char_p, vp, i64p, i32, i32]
    lib.dtts_finalize_weights.argtypes = [vp, i32]
    lib.dtts_text2mel_encode.argtypes = [vp] + [vp] * 8 + [i32] * 5 + [C.POINTER(C.c_int32), vp]
    lib.dtts_text2mel_decode.argtypes = [vp, vp, vp, vp]
    lib.dtts_text2mel_encode_ids.argtypes = [vp, vp, vp, vp, vp] + [i32] * 5 + [C.POINTER(C.c_int32), vp]
    lib.dtts_text2mel_speakers.argtypes = [vp, i32, vp, i32, vp]
    lib.dtts_dict_table_upload.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.dtts_text2mel_fetch.argtypes = [vp, i32, vp, vp]
    lib.dtts_hifigan_forward.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.dtts_length_regulate.argtypes = [vp, vp, vp, i32, i32, vp, i32, C.POINTER(C.c_int32), vp]
    lib.dtts_hifigan_hop.argtypes = [vp]
    lib.dtts_wav_to_int16.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    lib.dtts_text2mel_forward.argtypes = [vp] + [vp] * 8 + [i32, vp, i32, i32, i32, i32, i32, vp, i32, C.POINTER(C.c_int64), vp, vp, vp]
    lib.dtts_text2mel_forward_ids.argtypes = [vp] + [vp] * 4 + [i32, vp, i32, i32, i32, i32, i32, vp, i32, C.POINTER(C.c_int64), vp, vp, vp]
    lib.dtts_fft_blocks_forward.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.dtts_timer_enable.argtypes = [vp, i32]
    lib.dtts_timer_read.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.dtts_timer_reset.argtypes = [vp]
    lib.dtts_set_noise_seed.argtypes = [vp, C.c_uint64]
    lib.dtts_vocoder_range_guard.argtypes = [vp, i32]
    lib.dtts_vocoder_clamped.argtypes = [vp, C.POINTER(C.c_int64), i32, vp]
    lib.dtts_vocoder_nonfinite.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.dtts_vocoder_fp16_bound.argtypes = [vp, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.dtts_debug_check.argtypes = [vp, C.POINTER(C.c_int64), vp]
    lib.dtts_debug_poke.argtypes = [vp, vp]
    _lib = lib
    return lib


def default_config():
    cfg = DttsConfig()
    lib = load_library()
    if lib.dtts_config_sizeof() != C.sizeof(DttsConfig):
        raise DttsError(f"dtts_config layout mismatch: library {lib.dtts_config_sizeof()} B, abi.DttsConfig {C.sizeof(DttsConfig)} B")
    lib.dtts_default_config(C.byref(cfg))
    return cfg


class Context:
    """One dtts_handle (single owner, one per GPU / process)."""

    def __init__(self, cfg=None):
        self.lib = load_library()
        self.cfg = cfg or default_config()
        self.h = C.c_void_p()
        rc = self.lib.dtts_create(C.byref(self.cfg), C.byref(self.h))
        if rc != 0:
            raise DttsError(f"dtts_create failed ({rc}): {self.lib.dtts_last_error(None).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.dtts_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self.lib.dtts_last_error(self.h).decode()

    def _chk(self, rc, what):
        if rc != 0:
            raise DttsError(f"{what} failed ({rc}): {self.lib.dtts_last_error(self.h).decode()}")

    def load_state_dict(self, prefix, state):
        """state: mapping name -> numpy array or torch tensor (fp32); names are the reference's keys"""
        for k, v in state.items():
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            if a.dtype != np.float32:
                if not np.issubdtype(a.dtype, np.floating):
                    continue  # e.g. num_batches_tracked-style integer buffers: not part of this path
                a = a.astype(np.float32)
            a = np.ascontiguousarray(a)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._chk(self.lib.dtts_load_weight(self.h, f"{prefix}.{k}".encode(), a.ctypes.data_as(C.c_void_p), shape,
                                                a.ndim, DTTS_F32), f"dtts_load_weight({k})")

    def finalize(self, parts):
        self._chk(self.lib.dtts_finalize_weights(self.h, parts), "dtts_finalize_weights")

    def hop(self):
        return self.lib.dtts_hifigan_hop(self.h)

    def text2mel_encode(self, word_tokens, keys, values, key_map, pinyin, pinyin_map, pron_modified, mel2word, B, T_w,
                        L_k, P, stream):
        """all tensor arguments are device pointers (ints, 0/None = NULL); returns T_mel"""
        t_mel = C.c_int32(0)
        m2w_ptr, T_m2w = (mel2word if mel2word else (None, 0))
        self._chk(self.lib.dtts_text2mel_encode(self.h, word_tokens, keys, values, key_map, pinyin, pinyin_map,
                                                pron_modified or None, m2w_ptr, T_m2w, B, T_w, L_k, P, C.byref(t_mel),
                                                stream), "dtts_text2mel_encode")
        return t_mel.value

    def dict_table_upload(self, tok_off, keys, values, key_map, pin_off, pinyin, pinyin_map):
        """numpy arrays (host): tok_off/pin_off int32 [n+1], keys/values f32 [sum_L,768] (values may be None = keys),
        key_map f32 [sum_L], pinyin / pinyin_map int64 [sum_P]"""
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        tok_off, pin_off = c(tok_off, np.int32), c(pin_off, np.int32)
        keys, key_map = c(keys, np.float32), c(key_map, np.float32)
        values = None if values is None else c(values, np.float32)
        pinyin, pinyin_map = c(pinyin, np.int64), c(pinyin_map, np.int64)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.dtts_dict_table_upload(self.h, len(tok_off) - 1, p(tok_off), p(keys), p(values), p(key_map),
                                                  p(pin_off), p(pinyin), p(pinyin_map)), "dtts_dict_table_upload")

    def dict_table_edit(self, entry_id, tok_off, pin_off, key_map, pinyin, pinyin_map, keys, values, stream, rows_on_device=False):
        """replace / append entries of the resident table (dtts_text2mel_fetch(DTTS_DICT_EDIT); an administrative call: synchronous, one device
        synchronisation).  numpy arrays (host) for the edited entries only, laid out as dict_table_upload's: entry_id int32 [n] strictly
        ascending (< n_entries replaces, n_entries .. appends), tok_off / pin_off int32 [n + 1], key_map f32 [sum_L], pinyin / pinyin_map int64
        [sum_P].  keys / values: f32 [sum_L, gloss_dim] numpy arrays, or with rows_on_device DEVICE pointers (ints, 16-byte aligned) whose
        producer was enqueued on ``stream``; values may be None = keys"""
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        entry_id, tok_off, pin_off = c(entry_id, np.int32).reshape(-1), c(tok_off, np.int32).reshape(-1), c(pin_off, np.int32).reshape(-1)
        n = entry_id.shape[0]
        if tok_off.shape[0] != n + 1 or pin_off.shape[0] != n + 1:
            raise DttsError(f"dict_table_edit: {n} entries need n + 1 offsets, got {tok_off.shape[0]} / {pin_off.shape[0]}")
        key_map, pinyin, pinyin_map = c(key_map, np.float32), c(pinyin, np.int64), c(pinyin_map, np.int64)
        if not rows_on_device:
            keys = c(keys, np.float32)
            values = None if values is None else c(values, np.float32)
        p = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else int(a))
        a = dict_edit_args(n, p(entry_id), p(tok_off), p(pin_off), p(key_map), p(pinyin), p(pinyin_map), p(keys), p(values), rows_on_device)
        self._chk(self.lib.dtts_text2mel_fetch(self.h, DICT_EDIT, C.byref(a), stream), "dtts_text2mel_fetch(DTTS_DICT_EDIT)")

    def dict_table_entry(self, entry, stream, **dst):
        """what the resident table holds for an entry (dtts_text2mel_fetch(DTTS_DICT_ENTRY)) -> (n_entries, L_e, P_e), read from the context's
        host copy of the offsets; keywords: those of ``dict_entry_args`` — device destinations k / v f32 [L_e, hidden], key_map f32 [L_e],
        pinyin / pinyin_map i64 [P_e], filled by copies enqueued on ``stream``.  entry = -1: only the count"""
        a = dict_entry_args(entry, **dst)
        self._chk(self.lib.dtts_text2mel_fetch(self.h, DICT_ENTRY, C.byref(a), stream), "dtts_text2mel_fetch(DTTS_DICT_ENTRY)")
        return a.n_entries, a.L_e, a.P_e

    def text2mel_encode_ids(self, word_tokens, entry_ids, pron_modified, mel2word, B, T_w, L_k, P, stream):
        t_mel = C.c_int32(0)
        m2w_ptr, T_m2w = (mel2word if mel2word else (None, 0))
        self._chk(self.lib.dtts_text2mel_encode_ids(self.h, word_tokens, entry_ids, pron_modified or None, m2w_ptr, T_m2w, B,
                                                    T_w, L_k, P, C.byref(t_mel), stream), "dtts_text2mel_encode_ids")
        return t_mel.value

    def text2mel_speakers(self, kind, spk, B, stream):
        """project B speaker inputs (device pointer: fp32 [B,256] for SPK_EMBED, int64 [B] for SPK_ID) and arm the next encode"""
        self._chk(self.lib.dtts_text2mel_speakers(self.h, int(kind), spk, int(B), stream), "dtts_text2mel_speakers")

    def text2mel_decode(self, z_p, mel_out, stream):
        self._chk(self.lib.dtts_text2mel_decode(self.h, z_p, mel_out, stream), "dtts_text2mel_decode")

    def _fetch_block(self, what, block, stream):
        """dtts_text2mel_fetch of an item whose dst is a host argument block"""
        self._chk(self.lib.dtts_text2mel_fetch(self.h, what, C.byref(block), stream), f"dtts_text2mel_fetch({OUT_NAMES[what]})")

    def text2mel_posterior(self, tgt_mels, mel_ld, eps, eps_ld, mel_out, mel_cap, m_q, logs_q, z_p, kl, stream):
        """the teacher-forced FVAE posterior pass after an encode: dtts_text2mel_fetch(DTTS_OUT_POSTERIOR) with its host argument block
        (device pointers; eps / m_q / logs_q / z_p / kl may be None)"""
        a = PosteriorArgs(C.sizeof(PosteriorArgs), int(mel_ld), int(eps_ld), int(mel_cap), tgt_mels, eps, mel_out, m_q, logs_q, z_p, kl)
        self._fetch_block(OUT_POSTERIOR, a, stream)

    def melspec(self, wav, wav_lens, B, wav_ld, hop, mel, mel_cap, mel_lens, stream, eps=1e-6, lin=None):
        """log-mel spectrograms of B waveforms in one launch (dtts_text2mel_fetch(DTTS_OUT_MELSPEC); needs PART_MELSPEC finalised, no encode):
        device pointers wav f32 [B, wav_ld], wav_lens i32 [B] or None, mel f32 [B, mel_cap, n_mels] out, mel_lens i32 [B] out or None,
        lin f32 like mel or None: the mel values before the floor and the logarithm"""
        a = MelspecArgs(C.sizeof(MelspecArgs), int(hop), int(B), int(wav_ld), int(mel_cap), float(eps), wav, wav_lens or None, mel, mel_lens or None, lin or None)
        self._fetch_block(OUT_MELSPEC, a, stream)

    def stft_distance(self, x, y, lens, B, wav_ld, hops, sums, count, stream, mag=None, mag_cap=0):
        """the sums behind the multi-resolution STFT figures of B waveform pairs (dtts_text2mel_fetch(DTTS_OUT_STFT_DISTANCE); needs PART_STFT
        finalised, no encode): device pointers x, y f32 [B, wav_ld] (y the recording), lens i32 [B] or None, sums f64 [n_res, B, 3] out,
        count i64 [n_res, B] out, mag f32 or None (the clamped magnitudes, resolution after resolution [2, B, mag_cap, n_fft_i / 2 + 1]);
        hops: one hop per resolution, n_res = len(hops)"""
        hops = [int(v) for v in hops]
        if not 1 <= len(hops) <= 4:
            raise DttsError(f"stft_distance: {len(hops)} resolutions (supported: 1 .. 4)")
        a = StftArgs(C.sizeof(StftArgs), len(hops), (C.c_int32 * 4)(*hops), int(B), int(wav_ld), int(mag_cap), 0, x, y, lens or None, sums, count, mag or None)
        self._fetch_block(OUT_STFT_DISTANCE, a, stream)

    def spectral(self, mode, B, wav_ld, hop, spec_cap, stream, wav=None, lens=None, frames=None, spec=None, out=None, out_lens=None, floor=0.0):
        """STFT (mode SPECTRAL_FORWARD), inverse STFT (SPECTRAL_INVERSE) or STFT -> max(|S| - floor, 0) -> inverse STFT (both bits: the
        reference's denoise) of B waveforms (dtts_text2mel_fetch(DTTS_OUT_SPECTRAL); needs PART_ISTFT finalised, no encode).  Device
        pointers: wav f32 [B, wav_ld], lens i32 [B] or None, frames i32 [B], spec f32 [B, spec_cap, n_fft / 2 + 1, 2], out f32 [B, wav_ld],
        out_lens i32 [B] or None; with both bits spec and frames may be None (the context's workspace)."""
        a = SpectralArgs(C.sizeof(SpectralArgs), int(mode), int(hop), int(B), int(wav_ld), int(spec_cap), float(floor), wav or None, lens or None,
                         frames or None, spec or None, out or None, out_lens or None)
        self._fetch_block(OUT_SPECTRAL, a, stream)

    def griffin_lim(self, B, spec_cap, hop, n_iter, wav_ld, out, stream, mag=None, mel=None, n_mels=0, init=None, frames=None, out_lens=None,
                    spec_out=None):
        """Griffin-Lim of B magnitude (mag f32 [B, spec_cap, n_fft / 2 + 1]) or log10-mel (mel f32 [B, spec_cap, n_mels]; needs
        "istft.inv_mel_basis" in the plan) spectrograms (dtts_text2mel_fetch(DTTS_OUT_GRIFFIN_LIM); needs PART_ISTFT finalised, no encode).
        Device pointers: init f32 [B, spec_cap, n_fft / 2 + 1, 2] or None = zero phase, frames i32 [B] or None = spec_cap, out f32
        [B, wav_ld], out_lens i32 [B] or None, spec_out f32 like init or None: the spectrum `out` was inverted from."""
        a = GriffinLimArgs(C.sizeof(GriffinLimArgs), int(B), int(spec_cap), int(hop), int(n_iter), int(wav_ld), int(n_mels), 0, mag or None, mel or None,
                           init or None, frames or None, out or None, out_lens or None, spec_out or None)
        self._fetch_block(OUT_GRIFFIN_LIM, a, stream)

    def losses(self, B, stream, pred=None, tgt=None, T=0, n_mel=0, mel_sums=None, mel_count=None, pred_ld=0, tgt_ld=0, bias=6.0, ssim_map=None,
               dur_pred=None, mel2word=None, word_len=None, T_w=0, T_mel=0, m2w_ld=0, dur_scale=0, dur_sums=None, dur_gt=None):
        """the sums behind validation_step's losses of B utterances (dtts_text2mel_fetch(DTTS_OUT_LOSSES); needs no weights and no encode).
        Device pointers.  Mel half (runs iff mel_sums is given): pred f32 [B, pred_ld, n_mel], tgt f32 [B, tgt_ld, n_mel] (leading dimensions
        0 = T), mel_sums f64 [B, 3] out (sum w |p - t|, sum w (p - t)^2, sum w (1 - ssim)), mel_count i64 [B] out, ssim_map f32 [B, T, n_mel]
        out or None.  Duration half (runs iff dur_sums is given): dur_pred f32 [B, T_w], mel2word i64 [B, m2w_ld] with T_mel columns used,
        word_len i32 [B], dur_scale 0 = log / 1 = linear, dur_sums f64 [B, 5] out, dur_gt i32 [B, T_w] out or None."""
        a = LossArgs(C.sizeof(LossArgs), int(B), int(T), int(n_mel), int(pred_ld), int(tgt_ld), float(bias), int(T_w), int(T_mel), int(m2w_ld),
                     int(dur_scale), 0, pred or None, tgt or None, mel_sums or None, mel_count or None, ssim_map or None, dur_pred or None,
                     mel2word or None, word_len or None, dur_sums or None, dur_gt or None)
        self._fetch_block(OUT_LOSSES, a, stream)

    def dtw(self, B, stream, **kw):
        """dynamic time warping of B pairs (dtts_text2mel_fetch(DTTS_OUT_DTW); needs no weights and no encode).  Keywords: those of
        ``dtw_args`` — x [B, x_ld, F] and y [B, y_ld, F] of dtype 0 = f32 / 1 = f64, x_lens / y_lens i32 [B] or None, window (< 0: no
        band), slope, dist f64 [B] out, path i32 [B, 2, path_ld] + path_len i32 [B] out or None, acc f64 [B, x_ld, y_ld] out or None,
        moments f64 [B, 2, 4] out or None (F = 1)."""
        self._fetch_block(OUT_DTW, dtw_args(B, **kw), stream)

    def disc(self, B, stream, **kw):
        """HifiGAN's discriminators on B waveform pairs (dtts_text2mel_fetch(DTTS_OUT_DISC); needs PART_DISC finalised, no encode).  Keywords:
        those of ``disc_args`` — y, y_hat f32 [B, wav_ld], lens i32 [B] or None, which (DISC_MPD | DISC_MSD | DISC_FM), sums f64 [B, 8, 4],
        counts i64 [B, 8], status i32 [B] out, fm f64 [B, 8, 8] + fm_counts i64 [B, 8, 8] out (DISC_FM), d f32 [8, 2, B, d_ld] out or None."""
        self._fetch_block(OUT_DISC, disc_args(B, **kw), stream)

    def meldisc(self, n_sig, stream, **kw):
        """the multi-window mel discriminator on clips of n_sig mels (dtts_text2mel_fetch(DTTS_OUT_MELDISC); needs PART_MELDISC finalised, no
        encode).  Keywords: those of ``meldisc_args`` — mel f32 [n_sig, T_ld, 80], lens i32 [n_sig] or None, n_win, clips_ld, starts i32
        [n_win, n_sig, clips_ld] or None (then hop), reduction, flags, sums f64 [n_sig, 3, 2], counts i64 [n_sig, 3], status i32 [n_sig] out,
        d f32 [n_win, n_sig, clips_ld, 16] out or None, h 9 x f32 [n_sig, clips_ld, t, f, H] out or None."""
        self._fetch_block(OUT_MELDISC, meldisc_args(n_sig, **kw), stream)

    def spkenc(self, B, stream, **kw):
        """utterance embeddings of B recordings or mel sequences (dtts_text2mel_fetch(DTTS_OUT_SPKENC); needs PART_SPKENC finalised, no
        encode).  Keywords: those of ``spkenc_args`` — wav f32 [B, wav_ld] (SPKENC_FROM_MELS: mels f32 [B, wav_ld, 40]), lens i32 [B] or
        None, frame_step, min_coverage, pad_mode, tile_m, embed f32 [B, 256] and n_partials i32 [B] out, partials f32 [B, P, 256], mel f32
        [B, F, 40], hseq 3 x f32 [B, P, T, 256] out or None (P = spkenc_max_partials, F = spkenc_frames_ld)."""
        self._fetch_block(OUT_SPKENC, spkenc_args(B, **kw), stream)

    def pitch(self, B, stream, **kw):
        """F0 tracks of B waveforms (dtts_text2mel_fetch(DTTS_OUT_PITCH); needs no weights and no encode).  Keywords: those of
        ``pitch_args`` — wav f32 [B, wav_ld], lens i32 [B] or None, the analysis parameters, f0 f64 [B, frames_ld] and n_frames i32 [B] out,
        and the optional stage outputs acf f64 [B, frames_ld, n_lag], cand f64 [B, frames_ld, 15, 2], n_cand i32 [B, frames_ld], intensity
        f64 [B, frames_ld], selected i32 [B, frames_ld]."""
        self._fetch_block(OUT_PITCH, pitch_args(B, **kw), stream)

    def load_resample_filter(self, half_window, num_table):
        """the resampler's plan: half_window f64 [n_win] (the right half of the windowed sinc, n_win - 1 a multiple of num_table) and its
        table precision -> "resample.filter" / "resample.num_table" in fp64, then dtts_finalize_weights(DTTS_PART_RESAMPLE).  A context holds
        ONE filter; ``resample_filter_key`` says which (units that share a context compare it before a call)"""
        self.resample_filter_key = None
        for name, v in (("resample.filter", half_window), ("resample.num_table", [num_table])):
            a = np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1))
            shape = (C.c_int64 * 1)(a.shape[0])
            self._chk(self.lib.dtts_load_weight(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, 1, DTTS_F64), f"dtts_load_weight({name})")
        self.finalize(PART_RESAMPLE)
        self.resample_filter_key = resample_filter_key(half_window, num_table)

    def resample(self, B, stream, **kw):
        """band-limited resampling of B waveforms (dtts_text2mel_fetch(DTTS_OUT_RESAMPLE); needs PART_RESAMPLE finalised, no encode).
        Keywords: those of ``resample_args`` — wav f32 [B, wav_ld], lens i32 [B] or None, sr_in, sr_out, out f32 [B, out_ld] and out_lens
        i32 [B] out, out64 f64 [B, out_ld] or None: the accumulators before their one rounding."""
        self._fetch_block(OUT_RESAMPLE, resample_args(B, **kw), stream)

    def loudness(self, B, stream, **kw):
        """BS.1770 integrated loudness of B waveforms and, with mode=1, their normalisation (dtts_text2mel_fetch(DTTS_OUT_LOUDNESS); needs no
        weights and no encode).  Keywords: those of ``loudness_args`` — wav f32 [B, wav_ld], lens i32 [B] or None, sample_rate, target_lufs,
        lufs f64 [B], gain f64 [B] and status i32 [B] out, out f32 [B, wav_ld] (mode 1), z f64 [B, blocks_ld] and n_blocks i32 [B] or None."""
        self._fetch_block(OUT_LOUDNESS, loudness_args(B, **kw), stream)

    def fetch(self, what, dst, stream):
        self._chk(self.lib.dtts_text2mel_fetch(self.h, what, dst, stream), "dtts_text2mel_fetch")

    def length_regulate(self, dur, ilens, B, T_w, mel2word, cap, stream):
        t_max = C.c_int32(0)
        self._chk(self.lib.dtts_length_regulate(self.h, dur, ilens, B, T_w, mel2word, cap, C.byref(t_max), stream),
                  "dtts_length_regulate")
        return t_max.value

    def hifigan_forward(self, mel, lens, B, T, wav, stream):
        self._chk(self.lib.dtts_hifigan_forward(self.h, mel, lens or None, B, T, wav, stream), "dtts_hifigan_forward")

    def wav_to_int16(self, wav, lens, B, T, norm, out, stream):
        self._chk(self.lib.dtts_wav_to_int16(self.h, wav, lens or None, B, T, int(bool(norm)), out, stream), "dtts_wav_to_int16")

    def text2mel_forward(self, word_tokens, keys, values, key_map, pinyin, pinyin_map, pron_modified, mel2word, z_p, z_cap, B, T_w, L_k,
                         P, mel_out, mel_cap, pron_attn, dur, stream):
        """single call: mel2word = (ptr, T_m2w) or None; z_p = device ptr [B,latent,z_cap] or None; returns T_mel"""
        m2w, t_m2w = mel2word if mel2word else (None, 0)
        t_mel = C.c_int64(0)
        self._chk(self.lib.dtts_text2mel_forward(self.h, word_tokens, keys, values, key_map, pinyin, pinyin_map, pron_modified or None,
                                                 m2w, t_m2w, z_p or None, int(z_cap), B, T_w, L_k, P, mel_out, int(mel_cap),
                                                 C.byref(t_mel), pron_attn or None, dur or None, stream), "dtts_text2mel_forward")
        return t_mel.value

    def fft_blocks_forward(self, x, lens, pos_table, n_pos, B, T, y, stream):
        self._chk(self.lib.dtts_fft_blocks_forward(self.h, x, lens or None, pos_table or None, int(n_pos), B, T, y, stream),
                  "dtts_fft_blocks_forward")

    def gloss_encode(self, n_gloss, stream, **kw):
        """gloss embeddings of n_gloss glosses packed as one ragged sequence (dtts_text2mel_fetch(DTTS_GLOSS_ENCODE); needs PART_GLOSS finalised).  Keywords: those
        of ``gloss_args`` — ids i64 [sum_L], tok_off i32 [n_gloss + 1], sum_L, L_max (the longest gloss), out f32 [sum_L, hidden] and status
        i64 [2] out.  Synchronises the stream once (the offsets are checked on the host)."""
        a = gloss_args(n_gloss, **kw)
        self._chk(self.lib.dtts_text2mel_fetch(self.h, GLOSS_ENCODE, C.byref(a), stream), "dtts_text2mel_fetch(DTTS_GLOSS_ENCODE)")

    def ps_encode(self, B, T_ph, T_w, txt_tokens, ph2word, status, stream, mel2word=None, want_attn=True):
        """the PortaSpeech baseline's encode (dtts_text2mel_fetch(DTTS_PS_ENCODE); needs PART_PORTASPEECH finalised): device pointers txt_tokens /
        ph2word i64 [B, T_ph], status i64 [4] out, mel2word = (ptr, T_m2w) or None; returns T_mel.  Synchronises the stream once without
        mel2word; the caller reads ``status`` afterwards (``ps_status_error``)."""
        t_mel = C.c_int32(0)
        m2w, t_m2w = mel2word if mel2word else (None, 0)
        a = ps_args(B, T_ph, T_w, txt_tokens, ph2word, status, t_mel, m2w, t_m2w, want_attn)
        self._chk(self.lib.dtts_text2mel_fetch(self.h, PS_ENCODE, C.byref(a), stream), "dtts_text2mel_fetch(DTTS_PS_ENCODE)")
        return t_mel.value

    def timer_enable(self, which):
        self._chk(self.lib.dtts_timer_enable(self.h, which), "dtts_timer_enable")

    def timer_read(self, which):
        ms, n = C.c_double(0), C.c_int64(0)
        self._chk(self.lib.dtts_timer_read(self.h, which, C.byref(ms), C.byref(n)), "dtts_timer_read")
        return ms.value, n.value

    def timer_reset(self):
        self._chk(self.lib.dtts_timer_reset(self.h), "dtts_timer_reset")

    def set_noise_seed(self, seed):
        """seed of the device-side prior sample (z_p == NULL); contexts otherwise start from a time / pid / device dependent seed"""
        self._chk(self.lib.dtts_set_noise_seed(self.h, int(seed) & (2 ** 64 - 1)), "dtts_set_noise_seed")

    def vocoder_range_guard(self, enable):
        self._chk(self.lib.dtts_vocoder_range_guard(self.h, int(bool(enable))), "dtts_vocoder_range_guard")

    def debug_check(self, stream):
        """memory-safety mode (config.debug_redzone): red-zone bytes damaged so far (synchronises the stream); 0 = every kernel stayed
        inside its buffers.  The first damaged zone is named by last_error()."""
        n = C.c_int64(0)
        self._chk(self.lib.dtts_debug_check(self.h, C.byref(n), stream), "dtts_debug_check")
        return n.value

    def debug_poke(self, stream):
        """self-test of the memory-safety mode: damage one red-zone byte"""
        self._chk(self.lib.dtts_debug_poke(self.h, stream), "dtts_debug_poke")

    def vocoder_clamped(self, stream, reset=True):
        """activations the fp16 ResBlock operands could not represent since the last reset (synchronises the stream)"""
        n = C.c_int64(0)
        self._chk(self.lib.dtts_vocoder_clamped(self.h, C.byref(n), int(bool(reset)), stream), "dtts_vocoder_clamped")
        return n.value

    def vocoder_nonfinite(self):
        """cumulative count of non-finite pre-tanh samples the always-on conv_post detector saw (no synchronisation: valid for every
        forward whose stream the caller has synchronised with)"""
        n = C.c_int64(0)
        self._chk(self.lib.dtts_vocoder_nonfinite(self.h, C.byref(n)), "dtts_vocoder_nonfinite")
        return n.value

    def vocoder_fp16_bound(self, mel_abs_max=6.0):
        """(worst_case, rms_estimate) of the values the ResBlocks round to fp16 for |mel| <= mel_abs_max (dtts_vocoder_fp16_bound)"""
        wc, est = C.c_double(0), C.c_double(0)
        self._chk(self.lib.dtts_vocoder_fp16_bound(self.h, C.c_float(mel_abs_max), C.byref(wc), C.byref(est)), "dtts_vocoder_fp16_bound")
        return wc.value, est.value
