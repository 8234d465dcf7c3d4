"""What the reference-scoring tests (tests/test_ref_scoring_host.py, tests/test_gpu_ref_scoring.py) share.  Importing this module
touches neither a GPU nor the library."""
import numpy as np


def numpy_confusion(q, ref, n_ref=None):
    """C[2][R][S] as include/vbx_hip.h defines it (vbx_batch_set_reference), in NumPy."""
    q = np.asarray(q, dtype=np.float64)
    ref = np.asarray(ref)
    R = int(ref.max()) + 1 if n_ref is None else n_ref
    onehot = np.zeros((len(ref), R))
    onehot[np.arange(len(ref)), ref] = 1.0
    return np.stack([onehot.T @ q, onehot.T @ -np.log(q + np.nextafter(0, 1))])
