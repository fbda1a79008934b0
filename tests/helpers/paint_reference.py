"""The numpy reference of the painting from the labels (csrc/cc_paint.hip, HipEngine.paint_labels / paint_runs): every voxel gets
its label's entry of a look-up table, out[v] = lut[label[v]]; label 0 and labels at or beyond the table's length give 0.  numpy only."""
import numpy as np


def paint_by_label(labels, luts):
    """labels: an array of unsigned labels (any shape); luts: one look-up table indexed by label along its first axis - (n_lut,) or
    (n_lut, k) - or a list / tuple of such tables.  -> lut[labels] (the table's trailing axes appended), 0 where a label is 0 or
    >= n_lut; a list of them for a list of tables."""
    if isinstance(luts, (list, tuple)):
        return [paint_by_label(labels, lut) for lut in luts]
    lut = np.asarray(luts)
    labels = np.asarray(labels)
    if labels.dtype == np.int32:
        labels = labels.view(np.uint32)
    lab = labels.astype(np.uint64)
    n_lut = lut.shape[0]
    out = lut[np.minimum(lab, np.uint64(n_lut - 1)).astype(np.int64)]
    out[(lab >= np.uint64(n_lut)) | (lab == 0)] = 0
    return out
