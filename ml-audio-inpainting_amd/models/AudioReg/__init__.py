"""models/AudioReg of the reference (the autoregressive baseline of the model
comparison; MATLAB there): the gap-wise Janssen algorithm of
utils/janssen_inp.m as train.m drives it, on the GPU (ainp/janssen.py ->
csrc/janssen.hip), and the gap SDR of train.m:196 / model_eval.m:60."""
from ainp.janssen import gap_sdr, janssen_inpaint

__all__ = ["janssen_inpaint", "gap_sdr"]
