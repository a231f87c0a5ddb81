"""models/AudioReg of the reference (the autoregressive baselines of the model
comparison; MATLAB there): the gap-wise Janssen algorithm of
utils/janssen_inp.m, its window-wise form of utils/segmentation_inp.m (Hann,
rectangular and Tukey windows) and the forward/backward extrapolation of
utils/arinpaint.m as train.m drives them, with the "lpc" or the "arburg"
estimator, on the GPU (ainp/janssen.py -> csrc/janssen.hip,
csrc/janssen_windows.hip, csrc/ar_extrapolate.hip), and the gap SDR of
train.m:196 / model_eval.m:60."""
from ainp.janssen import ar_extrapolate, gap_sdr, janssen_inpaint, janssen_windowed

__all__ = ["janssen_inpaint", "janssen_windowed", "ar_extrapolate", "gap_sdr"]
