"""GPU: what destroyed handles give back.  One cycle builds and closes a Context, a Batch of every appearance model, an NN handle with its
graph index and a ParticleFilter, each driven through the entry points that allocate on demand; after the first cycles (the runtime's own
pools and code objects are then resident) the device's free memory must not keep falling."""
import ctypes

import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth
from mtf_amd.sm import ParticleFilter

pytestmark = pytest.mark.gpu

H, W, RES, B = 64, 96, 64, 8
CYCLES, SETTLED = 12, 3
# Free memory after cycle 12 may lie below free memory after cycle 3 by at most this much.  It is what the commit BEFORE the owner types
# (hand-kept free lists, which this cycle shows to be complete) loses under this very script: the largest value of three runs, 0 bytes in each.
# The smallest step in free memory seen in those runs -- the granule -- was 2 MiB (2097152 bytes): a leaked buffer smaller than the granule
# that shares one with live memory is below what this test sees (tests/test_owned_cpu.py covers that class); a lost batch is ~10 MB per cycle.
SLACK_BYTES = 0
SCORED = (L.AM_SSD, L.AM_NCC, L.AM_MI)   # the models the candidate scorer serves


def _hip_runtime():
    """the HIP runtime the library is linked against, as this process has it loaded"""
    mtf_amd._lib.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({l.split()[-1] for l in f if "libamdhip64" in l})
    assert paths, "libamdhip64 is not loaded"
    return ctypes.CDLL(paths[0])


def _free_bytes(rt):
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert rt.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _cycle(frames, raw, probe=None):
    probe = probe or (lambda: None)
    ctx = mtf_amd.Context(0)
    ctx.set_image(frames[0])
    ctx.preprocess(raw, ksize=5, sigma_x=1.5, resize_factor=0.5)
    ctx.keep_prev()
    ctx.set_image(frames[1])
    probe()
    rng = np.random.default_rng(5)
    src = rng.uniform(8, 56, (24, 2))
    ctx.estimate_warp_from_pts(L.SSM_HOMOGRAPHY, src, src + 1.5)
    ctx.estimate_optical_flow(np.array([[30.0, 30.0], [48.5, 24.0], [60.0, 40.0], [40.0, 34.5], [70.0, 30.0]]))
    probe()
    corners = np.stack([synth.square_corners(30 + 5 * t, 30 + (t % 3), 36) for t in range(B)])
    sm = mtf_amd.sm_desc(L.SM_ESM, max_iters=2, leven_marq=1)
    for am in (L.AM_SSD, L.AM_NCC, L.AM_MI, L.AM_SCV, L.AM_RSCV, L.AM_LSCV, L.AM_LRSCV, L.AM_SPSS):
        b = mtf_amd.Batch(ctx, am, L.SSM_HOMOGRAPHY, RES, RES, B)
        if am == L.AM_LSCV:
            b.set_lscv(2, 2, 8, 8)
        if am == L.AM_LRSCV:
            b.set_lrscv(2, 2, 8, 8)
        b.set_corners(corners)
        b.init_template(sm)
        b.set_region(corners + 0.25, sm)
        b.track(sm)
        b.track_trace(2)
        b.track(sm)
        if am in SCORED:
            b.score_candidates(rng.normal(0, 1e-3, (16, 8)))
        probe()
        b.close()
        probe()
    one = mtf_amd.Batch(ctx, L.AM_SSD, L.SSM_HOMOGRAPHY, RES, RES, 1)
    one.set_corners(corners[:1])
    one.initialize_pix_vals()
    h = one.nn_create(64)
    one.nn_build(h, [one.nn_desc(64, [0.01] * 8, seed=3)])
    one.nn_gnn_build(h, dict(degree=8))
    q = rng.uniform(16, 240, (2, one.nn_feature_size()))
    one.nn_search(h, q)
    one.nn_gnn_search(h, q)
    probe()
    one.nn_destroy(h)
    one.close()
    pf = ParticleFilter(ctx, L.SSM_HOMOGRAPHY, RES, RES, n_particles=64, seed=7, resampling_type=3, adaptive_resampling_thresh=0.5)
    pf.initialize(corners[0])
    pf.update()
    probe()
    pf.close()
    ctx.close()
    probe()


def test_destroyed_handles_give_their_memory_back():
    rt = _hip_runtime()
    frames = [synth.make_frame(H, W, seed=11), synth.make_frame(H, W, seed=12)]
    raw = np.clip(synth.make_frame(2 * H, 2 * W, seed=13), 0, 255).astype(np.uint8)
    seen, after = [], {}
    for k in range(1, CYCLES + 1):
        _cycle(frames, raw, probe=lambda: seen.append(_free_bytes(rt)))
        after[k] = _free_bytes(rt)
    steps = [abs(a - b) for a, b in zip(seen, seen[1:]) if a != b]
    lost = after[SETTLED] - after[CYCLES]
    print("free memory after each cycle: %s" % [after[k] for k in sorted(after)])
    print("lost between cycle %d and cycle %d: %d bytes; smallest step in free memory (the granule): %s bytes" %
          (SETTLED, CYCLES, lost, min(steps) if steps else "none seen"))
    assert lost <= SLACK_BYTES
