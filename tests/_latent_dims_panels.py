"""Input panels of the latent-dimension fixtures (tests/golden/latent_dims.npz): built from the committed simulator fixtures
and seeded NumPy, so that the tests regenerate them without the reference.  Shared by tests/golden/make_latent_dims_golden.py
and the latent-dimension tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# estimate_latent_dims settings (v_ratio, z0_dim, max_total_dim, min_z3_dim)
SETTINGS = [(0.7, 3, 64, 3), (0.9, 2, 64, 1), (0.5, 3, 4, 3), (0.95, 1, 8, 0), (0.3, 0, 64, 2)]
RATIOS = [round(0.05 * k, 2) for k in range(1, 20)]
N_SLICES = [5, 10, 20]
# panels whose reference estimate is recorded (the rank-deficient 'const' panel has only its PCA ratios: the reference's QR
# whitens with round-off there)
ESTIMATED = ["hi", "sun", "colangelo", "ties", "binary", "n7", "offset", "f64"]


def panels():
    """name -> (x [n,1], y [n,1], v [n,p]) as the reference would receive them."""
    out = {}
    with np.load(os.path.join(GOLDEN, "hirano_imbens_N2000_p20_seed0.npz")) as f:
        out["hi"] = (f["x"], f["y"], f["v"])
    with np.load(os.path.join(GOLDEN, "sun_colangelo.npz")) as f:
        out["sun"] = (f["sun_x"], f["sun_y"], f["sun_v"])
        out["colangelo"] = (f["colangelo_x"], f["colangelo_y"], f["colangelo_v"])
    rs = np.random.RandomState(20)
    v = rs.randn(1500, 8).astype(np.float32)
    x = (v[:, :2].sum(1, keepdims=True) + 0.5 * rs.randn(1500, 1)).astype(np.float32)
    y = np.round(x + v[:, 2:3] ** 2 + 0.3 * rs.randn(1500, 1), 1).astype(np.float32)       # tie-heavy outcome
    out["ties"] = (x, y, v)
    v = rs.randn(1000, 6).astype(np.float32)
    x = (v[:, 0:1] + rs.randn(1000, 1) > 0).astype(np.float32)                              # binary treatment
    y = (2 * x + v[:, 1:2] - v[:, 2:3] + 0.5 * rs.randn(1000, 1)).astype(np.float32)
    out["binary"] = (x, y, v)
    v = rs.randn(7, 3).astype(np.float32)
    out["n7"] = (rs.randn(7, 1).astype(np.float32), rs.randn(7, 1).astype(np.float32), v)
    sd = np.exp(rs.randn(10)).astype(np.float32)
    base = rs.randn(1200, 10).astype(np.float32) * sd
    v = (base + 1e4 * sd).astype(np.float32)                                               # column offsets of 1e4 sd
    x = (base[:, :3].sum(1, keepdims=True) / sd[:3].sum() + rs.randn(1200, 1)).astype(np.float32)
    y = (x + base[:, 4:5] / sd[4] + rs.randn(1200, 1)).astype(np.float32)
    out["offset"] = (x, y, v)
    v = rs.randn(900, 12) @ (np.eye(12) + 0.3 * rs.randn(12, 12))                          # float64 input
    x = v[:, :1] - v[:, 1:2] + rs.randn(900, 1)
    y = np.sin(x) + v[:, 2:3] + 0.2 * rs.randn(900, 1)
    out["f64"] = (x, y, v)
    v = rs.randn(800, 8).astype(np.float32)
    v[:, 3] = 2.5                                                                             # a constant column
    x = (v[:, :1] + rs.randn(800, 1)).astype(np.float32)
    y = (x + v[:, 1:2] + rs.randn(800, 1)).astype(np.float32)
    out["const"] = (x, y, v)
    return out
