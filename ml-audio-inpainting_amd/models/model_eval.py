"""Drop-in for models/model_eval.py: inpaint the test_samples
clips with a fixed 80 ms gap at 2.0 s and write the reconstructed audio.

Follows models/model_eval.py:23-227 step by step, on the MI355X kernels:
  load_model      (:23-46)  PConvUNet / StackedBLSTMCNN from a state_dict
                            (loaded with weights_only=True, not False), eval()
  inpaint         (:48-195) load_audio -> create_gap_mask(0.08 s at 2.0 s) ->
                            extract_spectrogram of the clean and gapped audio
                            (GPU STFT) ->
      gan:      log1p magnitudes, frame mask [s//hop, ceil(e/hop)) of 1=valid,
                G(impaired, mask) -> spectrogram_to_audio(output, phase=original
                phase) -- the generator's log1p-domain output goes to the ISTFT
                as the magnitude, as the reference passes it (:162-173);
      cnnlstm:  mask [time_to_frames(2.0), time_to_frames(2.08)) of 1=gap,
                log10(|X (1 - mask)| + 1e-9) of the ORIGINAL spectrogram,
                10 ** model.reconstruct_spectrogram(...) ->
                spectrogram_to_audio(..., phase=original phase) (:174-191);
                    -> save_audio (peak-normalised FLAC, native encoder)
  run_evaluation  (:198-227) every .flac of input_dir -> <name>_<type>_inpainted.flac
  inpaint_blind             not in the reference: the same two models without
                            the clean signal's phase -- features of the observed
                            samples only, one forward pass, then the
                            gap-constrained Griffin-Lim of ainp_gap_phase
  run_blind_evaluation      every .flac through inpaint_blind ->
                            <name>_<type>_blind_inpainted.flac and the gap SDRs,
                            comparable with the rows below
  run_janssen_evaluation    the same clips and gap through the autoregressive
                            baseline (models/AudioReg; the third row of
                            models/AudioReg/model_eval.m's SDR table) ->
                            <name>_janssen_inpainted.flac and the gap SDRs
  run_janssen_mask_evaluation  the same with several gaps per clip, gaps closer
                            than w filled together (janssen_inpaint_mask)
  run_ar_evaluation         any cell of models/AudioReg/train.m's table: Janssen
                            or forward/backward extrapolation, "lpc" or "arburg"
  run_spain_evaluation      the sparsity row they are compared against
                            (models/AudioReg/references/spain): A-SPAIN or S-SPAIN
  export_48k_pairs          the clean / restored pairs at 48 kHz that the
                            perceptual metrics of models/AudioReg/train.m take
                            (GPU polyphase resampler, ainp_resample_poly)
Spectrogram plots (:157-162,180-185) are out of scope (plotting).  The ISTFT
runs on the GPU (ainp_istft); output length hop * (T - 1), as librosa's.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE =os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(HERE)
for _p in (HERE, _PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import utils  # noqa: E402
from models.CNNBLSTM.model import StackedBLSTMCNN  # noqa: E402
from models.GAN.networks import PConvUNet  # noqa: E402

GAP_LEN_S = 0.08      # model_eval.py:64
GAP_START_S = 2.0     # model_eval.py:70

DEFAULT_ENC = [(64, 7, 2, 3), (128, 5, 2, 2), (256, 5, 2, 2),
               (512, 3, 2, 1), (512, 3, 2, 1), (512, 3, 2, 1), (512, 3, 2, 1)]


def load_config(config_path):
    import yaml
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def load_model(model_type, config_path, checkpoint_path, device):
    """model_eval.py:23-46."""
    print(f"Loading {model_type} model from {checkpoint_path}...")
    if model_type == "gan":
        cfg = load_config(config_path)
        g = cfg["model"]["generator"]
        model = PConvUNet(input_channels=g["input_channels"], mask_channels=g["mask_channels"],
                          output_channels=g["output_channels"],
                          enc_layer_cfg=g.get("enc_layer_cfg", DEFAULT_ENC)).to(device)
    elif model_type == "cnnlstm":
        model = StackedBLSTMCNN(config_path).to(device)
    else:
        raise ValueError(f"Unknown model type: {model_type}")
    sd = checkpoint_path if isinstance(checkpoint_path, dict) else \
        torch.load(checkpoint_path, weights_only=True, map_location=device)
    model.load_state_dict(sd)
    model.eval()
    return model


def _time_to_frames(t, sr, hop):
    """librosa.time_to_frames."""
    return int(np.asarray(t * sr).astype(int)) // hop


def inpaint(model, config_path, audio_path, output_path, device):
    """model_eval.py:48-195; returns the reconstructed audio (also written)."""
    if isinstance(model, PConvUNet):
        model_type = "gan"
    elif isinstance(model, StackedBLSTMCNN):
        model_type = "cnnlstm"
    else:
        raise ValueError("Unknown model type.")
    config = load_config(config_path)
    sp = config["data"]["spectrogram"]
    n_fft, hop, win = sp["n_fft"], sp["hop_length"], sp["win_length"]

    audio, sr = utils.load_audio(audio_path)
    mask_td, (gap_start_sample, gap_end_sample) = utils.create_gap_mask(
        len(audio), GAP_LEN_S, sr, gap_start_s=GAP_START_S)
    impaired_audio = audio * mask_td
    original_spectrogram = utils.extract_spectrogram(audio, n_fft=n_fft, hop_length=hop,
                                                     win_length=win)
    original_magnitude = np.log1p(np.abs(original_spectrogram))
    original_phase = np.angle(original_spectrogram)

    if model_type == "gan":
        impaired_spectrogram = utils.extract_spectrogram(impaired_audio, n_fft=n_fft,
                                                         hop_length=hop, win_length=win)
        impaired_magnitude = np.log1p(np.abs(impaired_spectrogram))
        gs = gap_start_sample // hop
        ge = int(np.ceil(gap_end_sample / hop))
        T = original_magnitude.shape[1]
        gs, ge = max(0, gs), min(T, ge)
        spec_mask = np.ones_like(original_magnitude, dtype=np.float32)
        if ge > gs:
            spec_mask[:, gs:ge] = 0
        imp_t = torch.from_numpy(impaired_magnitude.astype(np.float32)).to(device)[None, None]
        mask_t = torch.from_numpy(spec_mask).to(device)[None, None]
        with torch.no_grad():
            inpainted = model(imp_t, mask_t)[0, 0]
    else:
        spec_mask = np.zeros(original_spectrogram.shape, dtype=np.float32)
        fs = _time_to_frames(GAP_START_S, sr, hop)
        fe = _time_to_frames(2.08, sr, hop)           # model_eval.py:149
        spec_mask[:, fs:fe] = 1
        mask_t = torch.from_numpy(spec_mask).to(device)
        log_imp = np.log10(np.abs(original_spectrogram * (1 - spec_mask)) + 1e-9)
        log_imp_t = torch.from_numpy(log_imp.astype(np.float32))[None].to(device)
        with torch.no_grad():
            inpainted = (10 ** model.reconstruct_spectrogram(log_imp_t, mask_t))[0]
    y = utils.spectrogram_to_audio(inpainted.float().cpu().numpy(), phase=original_phase,
                                   phase_info=False, n_fft=n_fft, hop_length=hop,
                                   win_length=win)
    utils.save_audio(y, file_path=output_path, sample_rate=sr)
    return y


def run_evaluation(input_dir, output_dir, model_type, checkpoint, config_path):
    """model_eval.py:198-227."""
    if not os.path.isdir(input_dir):
        print(f"Error: Input directory not found: {input_dir}")
        return
    if not isinstance(checkpoint, dict) and not os.path.exists(checkpoint):
        print(f"Error: Checkpoint file not found: {checkpoint}")
        return
    os.makedirs(output_dir, exist_ok=True)
    if not torch.cuda.is_available():
        raise RuntimeError("model_eval runs on the MI355X kernels: no GPU visible")
    device = torch.device("cuda")
    model = load_model(model_type, config_path, checkpoint, device)
    flac_files = sorted(f for f in os.listdir(input_dir) if f.lower().endswith(".flac"))
    print(f"Found {len(flac_files)} .flac files in {input_dir}")
    outs = []
    for filename in flac_files:
        out = os.path.join(output_dir, f"{os.path.splitext(filename)[0]}_{model_type}_inpainted.flac")
        inpaint(model, config_path, os.path.join(input_dir, filename), out, device)
        outs.append(out)
    return outs


def _missing_runs(observed):
    """(start, length) of every run of missing samples of a bool mask."""
    d = np.diff(np.concatenate(([0], (~np.asarray(observed, bool)).view(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return [(int(s), int(e - s)) for s, e in zip(starts, ends)]


def blind_magnitudes(model, config_path, observed_audio, observed, sr=16000):
    """The target magnitudes inpaint_blind hands to the phase step: features of
    the zero-filled observed audio through the fused feature kernel
    (ops.stft_features, each model's own frame-mask convention, as its dataset
    builds them at training time), one forward pass, and the raw network output
    taken to the linear domain -- expm1(max(out, 0)) for the GAN (trained on
    log1p magnitudes), 10 ** out for the CNN-BLSTM (log10).  observed_audio
    float32 cuda [S]; observed bool [S] (host).  Returns float32 cuda [F, T]."""
    from ainp import ops
    sp = load_config(config_path)["data"]["spectrogram"]
    n_fft, hop, win = sp["n_fft"], sp["hop_length"], sp["win_length"]
    gan = isinstance(model, PConvUNet)
    if not gan and not isinstance(model, StackedBLSTMCNN):
        raise ValueError("Unknown model type.")
    x = (observed_audio * torch.from_numpy(np.asarray(observed, bool)).to(observed_audio.device)
         ).to(torch.float32).reshape(1, -1).contiguous()
    feat, fmask = None, None
    for k, (gs, gl) in enumerate(_missing_runs(observed) or [(0, 0)]):
        start = torch.tensor([gs], dtype=torch.int64, device=x.device)
        if gan:
            _, imp, _, m = ops.stft_features(x, start, gl, n_fft, hop, win, mode=ops.FEAT_GAN,
                                             sample_rate=sr,
                                             outputs=(False, k == 0, False, True))
            feat = imp if k == 0 else feat
            fmask = m if fmask is None else torch.minimum(fmask, m)     # 1 = valid
        elif k == 0:     # the CNN-BLSTM's forward pass takes no mask
            feat = ops.stft_features(x, start, gl, n_fft, hop, win, mode=ops.FEAT_CNNBLSTM,
                                     sample_rate=sr, outputs=(True, False, False, False))[0]
    F, T = feat.shape[-2:]
    with torch.no_grad():
        if gan:
            out = model(feat[None], fmask[None]).reshape(F, T)
            return torch.expm1(out.float().clamp_min(0.0)).contiguous()
        out = model(feat.unsqueeze(1)).reshape(F, T)
        return (10.0 ** out.float()).contiguous()


def inpaint_blind(model, config_path, audio, mask, device, n_iter=64, momentum=0.99, init=None,
                  sr=16000):
    """Restore a gapped signal with either network without the phase of the
    clean signal (not in the reference, whose inpaint() borrows it).

    audio [S] (numpy or tensor; only the samples where mask is nonzero are
    read), mask [S] nonzero = observed.  blind_magnitudes gives the target
    magnitudes A from the observed samples alone; gap_phase_fill
    (ainp_gap_phase) then finds a phase for the frames that touch the gap and
    new values for the missing samples, n_iter iterations with `momentum`,
    starting from zeros or, with init="janssen", from janssen_inpaint_mask's
    fill.  Observed samples come back unchanged.  Returns float64 [S], numpy
    for numpy input, else a tensor on `device`.

    Deliberately not kept: the reference hands the GAN's log1p-domain output to
    the ISTFT as if it were a magnitude (inpaint() keeps that).  Here A must be
    commensurate with the STFT of the observed samples around the gap, so the
    network output is always taken back to the linear domain first."""
    from ainp.gap_phase import gap_phase_fill
    if init not in (None, "janssen"):
        raise ValueError(f"init must be None or 'janssen', got {init!r}")
    as_numpy = not isinstance(audio, torch.Tensor)
    observed = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask) != 0
    x = torch.as_tensor(np.asarray(audio, np.float64) if as_numpy else audio).to(
        device, torch.float64).reshape(-1)
    obs_t = torch.from_numpy(observed).to(device)
    x = torch.where(obs_t, x, torch.zeros_like(x))
    if observed.all():
        return x.cpu().numpy() if as_numpy else x
    sp = load_config(config_path)["data"]["spectrogram"]
    A = blind_magnitudes(model, config_path, x.float(), observed, sr=sr)
    if init == "janssen":
        from models.AudioReg import janssen_inpaint_mask
        start = janssen_inpaint_mask([x.cpu().numpy()], [observed])[0]
        x = torch.where(obs_t, x, torch.from_numpy(np.asarray(start, np.float64)).to(device))
    y = gap_phase_fill(x, obs_t, A, sp["n_fft"], sp["hop_length"], sp["win_length"],
                       n_iter=n_iter, momentum=momentum)
    return y.cpu().numpy() if as_numpy else y


def run_blind_evaluation(input_dir, output_dir, model_type, checkpoint, config_path,
                         gaps=((GAP_START_S, GAP_LEN_S),), n_iter=64, momentum=0.99, init=None):
    """run_evaluation without the clean phase: every .flac of input_dir gets the
    gaps ((start_s, length_s) each; inpaint()'s one by default), goes through
    inpaint_blind and is written as <stem>_<model_type>_blind_inpainted.flac.
    Returns {filename: SDR over the missing samples in dB}, measured as
    run_ar_evaluation and run_spain_evaluation measure theirs: like them the
    model sees the observed samples only, so the rows compare."""
    if not os.path.isdir(input_dir):
        print(f"Error: Input directory not found: {input_dir}")
        return
    if not isinstance(checkpoint, dict) and not os.path.exists(checkpoint):
        print(f"Error: Checkpoint file not found: {checkpoint}")
        return
    if not torch.cuda.is_available():
        raise RuntimeError("model_eval runs on the MI355X kernels: no GPU visible")
    device = torch.device("cuda")
    model = load_model(model_type, config_path, checkpoint, device)

    def fill(clean, masks):
        return [inpaint_blind(model, config_path, c, m, device, n_iter=n_iter,
                              momentum=momentum, init=init) for c, m in zip(clean, masks)]

    return _evaluate_gap_filler(input_dir, output_dir, f"{model_type}_blind", fill,
                                gaps=tuple((float(s), float(g)) for s, g in gaps))


def _evaluate_gap_filler(input_dir, output_dir, suffix, fill,
                         gaps=((GAP_START_S, GAP_LEN_S),)):
    """What the signal-processing rows share: the clips with their gaps
    ((start_s, length_s) each; inpaint()'s one by default) go to
    fill(clean, masks) -> restored as one batch, the results to
    <stem>_<suffix>_inpainted.flac, the SDRs over all missing samples to the
    caller."""
    from models.AudioReg import gap_sdr
    if not os.path.isdir(input_dir):
        print(f"Error: Input directory not found: {input_dir}")
        return
    os.makedirs(output_dir, exist_ok=True)
    if not torch.cuda.is_available():
        raise RuntimeError("model_eval runs on the MI355X kernels: no GPU visible")
    flac_files = sorted(f for f in os.listdir(input_dir) if f.lower().endswith(".flac"))
    print(f"Found {len(flac_files)} .flac files in {input_dir}")
    clean, masks, srs = [], [], []
    for filename in flac_files:
        audio, sr = utils.load_audio(os.path.join(input_dir, filename))
        observed = np.ones(len(audio), bool)
        for start_s, length_s in gaps:
            mask_td, _ = utils.create_gap_mask(len(audio), length_s, sr, gap_start_s=start_s)
            observed &= mask_td > 0
        clean.append(audio.astype(np.float64))
        masks.append(observed)
        srs.append(sr)
    restored = fill(clean, masks) if clean else []
    sdrs = {}
    for filename, x, y, m, sr in zip(flac_files, clean, restored, masks, srs):
        out = os.path.join(output_dir, f"{os.path.splitext(filename)[0]}_{suffix}_inpainted.flac")
        utils.save_audio(y, file_path=out, sample_rate=sr)
        sdrs[filename] = gap_sdr(x, y, m)
    return sdrs


def run_janssen_evaluation(input_dir, output_dir, p=512, w=4096, maxit=20):
    """The AR baseline on the clips and the gap of inpaint(): run_ar_evaluation's
    "janssen" cell with the "lpc" estimator, written as <stem>_janssen_inpainted.flac.
    Returns {filename: gap SDR in dB} (models/AudioReg/model_eval.m:60)."""
    return run_ar_evaluation(input_dir, output_dir, algorithm="janssen", method="lpc", p=p, w=w,
                             maxit=maxit)


def run_janssen_mask_evaluation(input_dir, output_dir, gaps=((2.0, 0.08),), p=512, w=4096,
                                maxit=20, method="lpc"):
    """run_janssen_evaluation for a list of (start_s, length_s) gaps per clip:
    janssen_inpaint_mask fills them, gaps closer than w samples to one another
    together.  Each result is written as <stem>_janssen_mask[_arburg]_inpainted.flac.
    Returns {filename: SDR over all missing samples in dB}; with the default
    gap these are run_janssen_evaluation's figures."""
    from models.AudioReg import janssen_inpaint_mask
    from ainp.janssen import method_id
    return _evaluate_gap_filler(
        input_dir, output_dir, "janssen_mask" + ("_arburg" if method_id(method) else ""),
        lambda clean, masks: janssen_inpaint_mask(clean, masks, p=p, w=w, maxit=maxit,
                                                  method=method),
        gaps=tuple((float(s), float(g)) for s, g in gaps))


def run_janssen_windowed_mask_evaluation(input_dir, output_dir, gaps=((2.0, 0.08),), p=512,
                                         w=4096, a=1024, wtype="hann", maxit=20, method="lpc"):
    """run_janssen_mask_evaluation for the window-wise algorithm on the whole
    clip: janssen_windowed_mask fills a list of (start_s, length_s) gaps per
    clip, however many of them one window sees, with windows of shape wtype
    ("hann", "rect" or "tukey") of w samples every a samples.  Each result is
    written as <stem>_janssen_<wtype>_mask[_arburg]_inpainted.flac.  Returns
    {filename: SDR over all missing samples in dB}."""
    from models.AudioReg import janssen_windowed_mask
    from ainp.janssen import method_id, wtype_key
    key = wtype_key(wtype)
    return _evaluate_gap_filler(
        input_dir, output_dir, f"janssen_{key}_mask" + ("_arburg" if method_id(method) else ""),
        lambda clean, masks: janssen_windowed_mask(clean, masks, p=p, w=w, a=a, wtype=key,
                                                   maxit=maxit, method=method),
        gaps=tuple((float(s), float(g)) for s, g in gaps))


AR_ALGORITHMS = ("extrapolation", "janssen", "janssen_hann", "janssen_rect", "janssen_tukey")


def run_ar_evaluation(input_dir, output_dir, algorithm="janssen", method="lpc", p=512, w=4096,
                      maxit=20, a=1024):
    """One cell of models/AudioReg/train.m's table on the clips and the gap of
    inpaint(): algorithm "extrapolation", "janssen" (gap-wise) or "janssen_hann"
    / "janssen_rect" / "janssen_tukey" (window-wise, windows of w samples every
    a samples; a applies to these three only), estimator "lpc" or "arburg".
    Every .flac of input_dir gets the 80 ms gap at 2.0 s, all gaps are filled
    in one batch, and each result is written as
    <stem>_<algorithm>[_arburg]_inpainted.flac.  Returns {filename: gap SDR in
    dB}, measured before save_audio's normalisation and 16-bit quantisation.
    maxit does not apply to "extrapolation"."""
    from models.AudioReg import ar_extrapolate, janssen_inpaint, janssen_windowed
    from ainp.janssen import method_id
    if algorithm not in AR_ALGORITHMS:
        raise ValueError(f"algorithm must be one of {AR_ALGORITHMS}, got {algorithm!r}")
    suffix = algorithm + ("_arburg" if method_id(method) else "")

    def fill(clean, masks):
        if algorithm == "janssen":
            return janssen_inpaint(clean, masks, p=p, w=w, maxit=maxit, method=method)
        if algorithm.startswith("janssen_"):
            return janssen_windowed(clean, masks, p=p, w=w, a=a, maxit=maxit, method=method,
                                    wtype=algorithm[len("janssen_"):])
        return ar_extrapolate(clean, masks, p=p, w=w, method=method)

    return _evaluate_gap_filler(input_dir, output_dir, suffix, fill)


SPAIN_ALGORITHMS = ("aspain", "sspain")


def run_spain_evaluation(input_dir, output_dir, algorithm="aspain", w=4096, a=1024, **solver):
    """The sparsity row of the same comparison (references/spain) on the clips
    and the gap of inpaint(): algorithm "aspain" or "sspain", Hann windows of w
    samples every a samples, **solver handed to spain_inpaint (red, s, r,
    epsilon, maxit, f_update, omp_errdb).  Every .flac of input_dir gets the
    80 ms gap at 2.0 s, all gaps are filled in one batch, and each result is
    written as <stem>_<algorithm>_inpainted.flac, <stem>_sspain_omp_inpainted.flac
    with f_update "OMP".  Returns {filename: gap SDR in dB}, measured before
    save_audio's normalisation and 16-bit quantisation."""
    from models.AudioReg import spain_inpaint
    if algorithm not in SPAIN_ALGORITHMS:
        raise ValueError(f"algorithm must be one of {SPAIN_ALGORITHMS}, got {algorithm!r}")
    f_update = solver.get("f_update", "H")
    omp = isinstance(f_update, str) and f_update.upper() == "OMP"
    return _evaluate_gap_filler(
        input_dir, output_dir, algorithm + ("_omp" if omp else ""),
        lambda clean, masks: spain_inpaint(clean, masks, algorithm=algorithm, w=w, a=a, **solver))


def run_spain_learned_evaluation(input_dir, output_dir, basis=None, algorithm="aspain", w=1024,
                                 a=256, **solver):
    """SPAIN over the whole signal (references/basisopt: a_spain_learned.m /
    s_spain_learned.m) on the clips and the gap of inpaint(): algorithm "aspain"
    or "sspain", the Gabor frame of a Hann window of w samples every a samples,
    basis None (the global SPAIN row), a unitary [K, K] matrix or "learn" / a
    dict of learning options (the learned row; "learn": one basis per clip from
    its own reliable frames, as spain_learned_inpaint learns it), **solver handed
    to spain_learned_inpaint (M, s, r, epsilon, maxit).
    Each result is written as <stem>_<algorithm>_global_inpainted.flac without a
    basis and <stem>_<algorithm>_learned_inpainted.flac with one.  Returns
    {filename: gap SDR in dB}, measured as run_spain_evaluation measures it."""
    from models.AudioReg import spain_learned_inpaint
    if algorithm not in SPAIN_ALGORITHMS:
        raise ValueError(f"algorithm must be one of {SPAIN_ALGORITHMS}, got {algorithm!r}")
    return _evaluate_gap_filler(
        input_dir, output_dir, f"{algorithm}_{'global' if basis is None else 'learned'}",
        lambda clean, masks: spain_learned_inpaint(clean, masks, basis=basis, algorithm=algorithm,
                                                   w=w, a=a, **solver))


EXPORT_SR = 48000     # models/AudioReg/train.m:72, model_eval.m:68: what PEMO-Q and PEAQ take


def export_48k_pairs(input_dir, reconstructed_dir, output_dir, suffix):
    """models/AudioReg/train.m:72-73,203-204 (model_eval.m:68-71): the clean and
    the restored signal resampled to 48 kHz for the perceptual metrics.  For
    every <stem>.flac of input_dir with a <stem>_<suffix>_inpainted.flac in
    reconstructed_dir, writes <stem>_signal.wav and <stem>_<suffix>_solution.wav
    to output_dir: 48 kHz, resampled in float64 on the GPU, all clips of one
    native rate in one launch, saved without normalisation as audiowrite saves
    them.  Returns the list of (signal path, solution path).  PEMO-Q and PEAQ
    themselves are closed toolboxes and stay out of scope."""
    from ainp import ops
    if not os.path.isdir(input_dir):
        print(f"Error: Input directory not found: {input_dir}")
        return []
    if not torch.cuda.is_available():
        raise RuntimeError("model_eval runs on the MI355X kernels: no GPU visible")
    os.makedirs(output_dir, exist_ok=True)
    jobs, by_rate = [], {}     # (clip, output path); rows of jobs per native rate
    pairs = []
    for filename in sorted(f for f in os.listdir(input_dir) if f.lower().endswith(".flac")):
        stem = os.path.splitext(filename)[0]
        restored = os.path.join(reconstructed_dir, f"{stem}_{suffix}_inpainted.flac")
        if not os.path.exists(restored):
            continue
        outs = (os.path.join(output_dir, f"{stem}_signal.wav"),
                os.path.join(output_dir, f"{stem}_{suffix}_solution.wav"))
        for path, out in zip((os.path.join(input_dir, filename), restored), outs):
            try:
                data, sr = utils._read_any(path)
            except Exception as e:
                raise IOError(f"Error loading audio file {path}: {str(e)}")
            by_rate.setdefault(int(sr), []).append(len(jobs))
            jobs.append((data.mean(axis=1).astype(np.float64), out))
        pairs.append(outs)
    for sr, rows in by_rate.items():
        g = math.gcd(sr, EXPORT_SR)
        n = [len(jobs[k][0]) for k in rows]
        stride = max(2, -(-max(n) // 2) * 2)     # rows stay 16-byte aligned
        host = np.zeros((len(rows), stride), dtype=np.float64)
        for j, k in enumerate(rows):
            host[j, :n[j]] = jobs[k][0]
        y = ops.resample_poly(torch.from_numpy(host).cuda(), EXPORT_SR // g, sr // g, n=n).cpu()
        for j, k in enumerate(rows):
            n_out = -(-n[j] * (EXPORT_SR // g) // (sr // g))
            utils.save_audio(y[j, :n_out].numpy(), file_path=jobs[k][1], sample_rate=EXPORT_SR,
                             normalize=False, file_format="wav")
    return pairs


def run_stoi_evaluation(input_dir, reconstructed_dir, suffix, extended=False):
    """The intelligibility column of models/AudioReg/train.m:35-41 in place of
    the closed PEMO-Q / PEAQ toolboxes: STOI (extended: ESTOI) of every
    <stem>.flac of input_dir against its <stem>_<suffix>_inpainted.flac in
    reconstructed_dir, paired as export_48k_pairs pairs them.  Each pair is
    mixed to mono and truncated to the shorter of the two; all pairs of one
    native rate are scored in one call (ainp.stoi.stoi: one resampling launch to
    10 kHz, one scoring launch).  Returns {filename: score}."""
    from ainp.stoi import stoi
    if not os.path.isdir(input_dir):
        print(f"Error: Input directory not found: {input_dir}")
        return {}
    if not torch.cuda.is_available():
        raise RuntimeError("model_eval runs on the MI355X kernels: no GPU visible")
    by_rate = {}      # native rate -> [(filename, clean, restored)]
    for filename in sorted(f for f in os.listdir(input_dir) if f.lower().endswith(".flac")):
        stem = os.path.splitext(filename)[0]
        restored = os.path.join(reconstructed_dir, f"{stem}_{suffix}_inpainted.flac")
        if not os.path.exists(restored):
            continue
        pair = []
        for path in (os.path.join(input_dir, filename), restored):
            try:
                data, sr = utils._read_any(path)
            except Exception as e:
                raise IOError(f"Error loading audio file {path}: {str(e)}")
            pair.append((data.mean(axis=1).astype(np.float64), int(sr)))
        if pair[0][1] != pair[1][1]:
            raise ValueError(f"{filename}: clean at {pair[0][1]} Hz, restored at {pair[1][1]} Hz")
        n = min(len(pair[0][0]), len(pair[1][0]))
        by_rate.setdefault(pair[0][1], []).append((filename, pair[0][0][:n], pair[1][0][:n]))
    scores = {}
    for sr, rows in by_rate.items():
        got = stoi([c for _, c, _ in rows], [r for _, _, r in rows], fs=sr, extended=extended)
        for (filename, _, _), v in zip(rows, got):
            scores[filename] = float(v)
            print(f"{filename}: {'ESTOI' if extended else 'STOI'} {v:.4f}")
    return scores


if __name__ == "__main__":
    # model_eval.py:229-256 (CNN-LSTM configuration by default)
    run_evaluation(input_dir=sys.argv[1] if len(sys.argv) > 1 else "../test_samples",
                   output_dir=sys.argv[2] if len(sys.argv) > 2 else "../test_samples_reconstructed",
                   model_type=sys.argv[3] if len(sys.argv) > 3 else "cnnlstm",
                   checkpoint=sys.argv[4] if len(sys.argv) > 4 else
                   "CNNBLSTM/checkpoints/blstm_cnn_epoch_75.pt",
                   config_path=sys.argv[5] if len(sys.argv) > 5 else "CNNBLSTM/cnn_blstm.yaml")
