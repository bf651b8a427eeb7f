"""Generate tests/golden/latent_dims.npz by IMPORTING the reference (run in the build container only).

    python tests/golden/make_latent_dims_golden.py

Records the reference's estimate_latent_dims, get_SDR_dim (a sweep of ratio x n_slices, which pins the shape of its cumulative
SIR spectrum), slice_y and scikit-learn's PCA explained-variance ratios on the panels of tests/_latent_dims_panels.py.  The
fixture is data; the reference source never enters this repository and never travels to the GPU box.
"""
import os
import sys
import warnings

import numpy as np

REF = "/root/reference/src"
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    from bayesgm.utils.helpers import estimate_latent_dims, get_SDR_dim, slice_y
    from _latent_dims_panels import ESTIMATED, N_SLICES, RATIOS, SETTINGS, panels

    out = {}
    warnings.simplefilter("ignore")
    for name, (x, y, v) in panels().items():
        out[name + "_pca_ratio"] = PCA().fit(StandardScaler().fit_transform(v)).explained_variance_ratio_
        for ns in N_SLICES:
            ind, cnt = slice_y(np.sort(y[:, 0]), ns)
            out["%s_slice_y_%d_ind" % (name, ns)] = ind.astype(np.int16)
            out["%s_slice_y_%d_cnt" % (name, ns)] = cnt
        if name not in ESTIMATED:
            continue
        out[name + "_estimate"] = np.array([estimate_latent_dims(x, y, v, *s) for s in SETTINGS], dtype=np.int32)
        for target, t in (("y", y), ("x", x)):
            out["%s_sdr_%s" % (name, target)] = np.array([[get_SDR_dim(v, t, ns, r) for r in RATIOS] for ns in N_SLICES],
                                                         dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "latent_dims.npz"), **out)
    print("latent_dims.npz written to", HERE, "(%d arrays)" % len(out))


if __name__ == "__main__":
    main()
