"""The shared cases of the NN search / tracker tests (tests/test_nn_ref.py, tests/test_gpu_nn_search.py, tests/test_gpu_nn_tracker.py)."""
import numpy as np

import nn_ref as R

# ---- search alone: random matrices handed over through set_dataset ----
# (resx, resy, channels): feat_size 49 and 625 odd (every second row starts 8 bytes off a 16-byte boundary), 576 and 192 even, 7500 the
# largest row the issue names (50 x 50 x 3)
SEARCH_SHAPES = [(7, 7, 1), (24, 24, 1), (25, 25, 1), (8, 8, 3), (50, 50, 3)]
# fewer rows than a workgroup has waves, one under / at / over a wave's worth, more than one workgroup with a ragged last one, many
SEARCH_N = [1, 63, 64, 65, 257, 1000]
SEARCH_Q = [1, 3]


def search_matrix(feat_size, am, seed=5):
    """1000 random rows: SSD pixel values in [0, 255); NCC centred and of unit norm, as updateDistFeat writes them"""
    rng = np.random.default_rng(seed + feat_size)
    m = rng.uniform(0.0, 255.0, size=(1000, feat_size))
    return unit_rows(m) if am == R.NCC else m


def unit_rows(m):
    m = m - m.mean(axis=-1, keepdims=True)
    return m / np.linalg.norm(m, axis=-1, keepdims=True)


def planted_positions(n):
    """the first row, the last row, the last row of the last complete group of four (a workgroup's waves take four consecutive rows)"""
    return sorted({0, n - 1, max(0, (n // 4) * 4 - 1)})


def search_queries(m, n, pos, am, seed):
    """three queries against m[:n] (a call with Q = 1 takes the first): the first close to row pos (noise far below the rows' spread), the
    others close to rows drawn at random"""
    rng = np.random.default_rng(seed)
    rows = [pos] + [int(r) for r in rng.integers(0, n, size=2)]
    scale = 0.5 if am == R.SSD else 0.01 / np.sqrt(m.shape[1])
    q = m[rows] + rng.normal(0.0, scale, size=(3, m.shape[1]))
    return unit_rows(q) if am == R.NCC else q


# ---- the tracker: (id, am, ssm, res, channels, frames, max_iters, epsilon, seed) ----
SIGMA_H = np.array([0.01, 0.01, 1.0, 0.01, 0.01, 1.0, 5e-5, 5e-5])
SIGMA_A = np.array([1.0, 1.0, 0.01, 0.01, 0.01, 0.01])
N_SAMPLES = 200
TRACK_CASES = [
    ("ssd-hom-1", 0, 0, 24, 1, "frame2", 1, 0.0, 3),
    ("ssd-hom-5", 0, 0, 24, 1, "frame2", 5, 0.0, 3),
    ("ssd-hom-5-stop", 0, 0, 24, 1, "frame2", 5, 1e9, 3),
    ("ncc-hom-5", 1, 0, 24, 1, "frame2", 5, 0.0, 4),
    ("ssd-aff-5", 0, 1, 24, 1, "frame2", 5, 0.0, 5),
    ("ncc-aff-1", 1, 1, 24, 1, "frame2", 1, 1e9, 6),
    ("ssd-hom-25", 0, 0, 25, 1, "frame2", 5, 0.0, 7),
    ("ssd-hom-mc", 0, 0, 24, 3, "mc", 5, 0.0, 8),
]


def track_corners(res):
    from mtf_amd import synth
    return synth.square_corners(250.0, 262.0, 90.0) + np.random.default_rng(res).uniform(-2, 2, size=(2, 4))


def track_perturbations(ssm, seed):
    rng = np.random.default_rng(seed)
    S = 8 if ssm == 0 else 6
    p = rng.normal(size=(N_SAMPLES, S)) * (SIGMA_H if S == 8 else SIGMA_A)
    p[0] = 0.0            # (the zero perturbation is row 0)
    return p


def track_frames(kind, frame, frame2):
    """(the frame the dataset is built on, the frame tracked)"""
    if kind == "mc":
        from mtf_amd import synth
        a = synth.make_frame_mc(256, 256)
        b = np.ascontiguousarray(np.roll(a, (1, 2), axis=(0, 1)))      # the scene moved by one row and two columns
        return a, b
    return frame, frame2


def track_corners_for(kind, res):
    if kind == "mc":
        from mtf_amd import synth
        return synth.square_corners(128.0, 120.0, 70.0) + np.random.default_rng(res).uniform(-1, 1, size=(2, 4))
    return track_corners(res)
