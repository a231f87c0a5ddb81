"""models/AudioReg of the reference (the signal-processing rows of the model
comparison; MATLAB there): the gap-wise Janssen algorithm of
utils/janssen_inp.m (janssen_inpaint: one gap per segment; janssen_inpaint_mask:
any mask, csrc/janssen_mask.hip), its window-wise form of utils/segmentation_inp.m (Hann,
rectangular and Tukey windows; janssen_windowed: on train.m's per-gap support, one
gap per window; janssen_windowed_mask: on the whole signal as segmentation_inp.m is
written, any mask) and the forward/backward extrapolation of
utils/arinpaint.m as train.m drives them, with the "lpc" or the "arburg"
estimator, on the GPU (ainp/janssen.py -> csrc/janssen.hip,
csrc/janssen_windows.hip, csrc/ar_extrapolate.hip); the sparsity-based A-SPAIN
and S-SPAIN of references/spain (ainp/spain.py -> csrc/spain.hip between the
same gather and overlap-add) and their whole-signal form with a learned
unitary basis of references/basisopt (ainp/spain_learned.py ->
csrc/spain_learned.hip), the basis itself learned as basis_opt_new.m learns it
(ainp/basis_learn.py -> csrc/basis_learn.hip); the gap SDR of train.m:196 /
model_eval.m:60; and, for the intelligibility column the reference fills with
closed toolboxes, STOI / ESTOI of a batch and of every iteration of a Janssen
history (ainp/stoi.py -> csrc/stoi.hip)."""
from ainp.janssen import (ar_extrapolate, gap_sdr, janssen_inpaint, janssen_inpaint_mask,
                          janssen_windowed, janssen_windowed_mask, plan_mask_segments)
from ainp.basis_learn import learn_basis, spain_learn_basis, spain_training_frames
from ainp.spain import spain_inpaint
from ainp.spain_learned import spain_learned_inpaint
from ainp.stoi import stoi, stoi_curve

__all__ = ["janssen_inpaint", "janssen_inpaint_mask", "plan_mask_segments", "janssen_windowed", "janssen_windowed_mask", "ar_extrapolate", "spain_inpaint", "gap_sdr",
           "spain_learned_inpaint", "learn_basis", "spain_learn_basis", "spain_training_frames", "stoi", "stoi_curve"]
