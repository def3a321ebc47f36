"""nt::NN's dataset kernels (kernels_nn.hip) at the row lengths, grids and call orders tests/test_gpu_nn.py never reaches, against float64
references that run on the CPU: the oracle's generateDataset and -- homography, so that oracle and kernel are not held only to each other --
the independent NumPy walk oracle/numpy_ref.nn_dataset_rows (nn_mi_dist_feat for MI rows).

k_nn_rows (MATH_FAST, the two-launch form) works in PAIRS of entries, pair-rounds of 128 entries and chunks of 24 pair-rounds (3072 entries):
    R   = ceil(N / 128)            pair-rounds of the row
    Rc  = min(R - c0, 24)          pair-rounds of the chunk that starts at pair-round c0
    R4  = ceil(Rc / 4)             pair-rounds per wave in that chunk
    E   = 2 R4                     entries a lane holds in that chunk
    LDS = 512 ceil(min(R, 24) / 4) entries of 16 bytes (unit-z grid) or 24 bytes (x, y, z: a homography template whose corners are a
                                   general quadrilateral)
The shapes (resx, resy), and what each one is there for:
    51 x 49 = 2499   odd N below one chunk: R 20, Rc 20, R4 5, E 10; LDS 2560 entries = 40 KB unit-z / 60 KB not.  The narrow-store branch
                     (rows start on 8-byte boundaries only, the last pair has ONE valid entry); MI rows of 5 N doubles
    54 x 50 = 2700   even N in (2560, 3072): R 22, Rc 22, R4 6, E 12; LDS 3072 entries = 48 KB / 72 KB (above the 64 KB a launch gets
                     without the kernel's attribute); wave 3's last two pair-rounds are past the row's end
    64 x 48 = 3072   exactly one full chunk: R 24, Rc 24, R4 6, E 12; 48 KB / 72 KB; no tail at all; the last row length NCC takes through
                     the two-launch form
    59 x 53 = 3127   odd N, a second chunk of ONE pair-round: R 25; chunk 0 as 64 x 48, chunk 1: c0 24, Rc 1, R4 1, E 2 -- waves 1-3 idle,
                     the barrier in front of the LDS refill; 48 KB / 72 KB.  NCC: above 3072, the workgroup form (nn_two_launch_ok)
    80 x 80 = 6400   two full chunks and a ragged one: R 50; chunks 0, 1 full, chunk 2: c0 48, Rc 2, R4 1, E 2 -- waves 2, 3 idle; 48 / 72 KB.
                     NCC (workgroup form): above the 4096 entries a workgroup keeps in registers, the re-read path of k_nn_dataset
    81 x 79 = 6399   its odd neighbour: the same walk, the last pair of the last chunk has one valid entry
    128 x 25 = 3200  strongly non-square, even: R 25, chunk 1 of one pair-round (Rc 1, R4 1, E 2); 48 / 72 KB
MATH_REPLAY sends every row to the workgroup form k_nn_dataset (no pairs, no chunks: strides of 256 entries, NCC keeps 16 per thread), which
has not seen an odd or a long row either.

Grids: "homq" homography, general-quadrilateral corners (not unit-z: 24 bytes per LDS entry, no hull); "homsq" homography, exactly square
corners (unit-z, 16 bytes, the hull / all_inside shortcut live); "aff" affine (always unit-z, no division).  Positions: "inside" the frame,
and "border" (a third or more of the samples read the border value 128; waves with inside and outside lanes).

The cells (CELLS below) are the cross product pruned to what distinguishes code paths -- sample_batch (grid, position) is shared by the AMs,
the stores and the NCC sums are shared by the grids:
    MATH_FAST    every (shape, AM) at (homq, inside) [24-byte LDS, 60 / 72 KB], (homsq, border) [hull test fails for part of the samples:
                 both bodies of k_nn_rows, mixed waves] and (aff, inside); SSD additionally at (homq, border), (homsq, inside) [every
                 sample all_inside] and (aff, border)
    MATH_REPLAY  every (shape, AM) at (homq, border) and (aff, inside)
Every cell writes its rows through nn_dataset_dev into the middle of a sentinel-filled buffer and checks the guards on both sides: a pair
store that runs one entry past an odd row lands in the NEXT row, which the kernel then overwrites -- only the last row's overrun shows, and
only in a guard."""
import numpy as np
import pytest

import mtf_amd
from mtf_amd import _lib as L
from mtf_amd import synth
from mtf_amd.sm import NNDataset

pytestmark = pytest.mark.gpu

SIGMA_H = np.array([0.02, 0.02, 2.0, 0.02, 0.02, 2.0, 1e-4, 1e-4])
SIGMA_A = np.array([2.0, 2.0, 0.02, 0.02, 0.02, 0.02])

SHAPES = [(51, 49), (54, 50), (64, 48), (59, 53), (80, 80), (81, 79), (128, 25)]
AMS = {"ssd": (L.AM_SSD, {}), "ncc": (L.AM_NCC, {}), "mi8": (L.AM_MI, {}), "mi10pou": (L.AM_MI, dict(mi_n_bins=10, mi_pou=1))}
N_SAMPLES = 24
MI_INTEGER_MARGIN = 1e-7          # the reference's normalised pixel values stay this far from an integer: floor() is then the same on both sides
SENTINEL, GUARD = -7777.25, 4096


def _cells():
    out = []
    for shape in SHAPES:
        for am in AMS:
            out += [("fast", shape, am, "homq", "inside"), ("fast", shape, am, "homsq", "border"), ("fast", shape, am, "aff", "inside")]
            if am == "ssd":
                out += [("fast", shape, am, "homq", "border"), ("fast", shape, am, "homsq", "inside"), ("fast", shape, am, "aff", "border")]
            out += [("replay", shape, am, "homq", "border"), ("replay", shape, am, "aff", "inside")]
    return out


CELLS = _cells()


def _cell_id(c):
    return "%s-%dx%d-%s-%s-%s" % (c[0], c[1][0], c[1][1], c[2], c[3], c[4])


def case_inputs(frame, shape, grid, where):
    """(corners, perturbations) of a cell: seeded by shape, grid and position only, so that the AMs and the math modes of one geometry see the
    same samples.  The seed's base was chosen ON THE REFERENCE (test_nn_shapes_cpu.py asserts it): no normalised pixel value of any cell
    within MI_INTEGER_MARGIN of an integer."""
    h, w = frame.shape[:2]
    seed = 4000 + 100 * SHAPES.index(shape) + 10 * ("homq", "homsq", "aff").index(grid) + ("inside", "border").index(where)
    rng = np.random.default_rng(seed)
    corners = synth.square_corners(w / 2, h / 2, 100) if where == "inside" else synth.square_corners(w - 40.0, 35.0, 100)
    jitter = rng.uniform(-2, 2, size=(2, 4))
    if grid != "homsq":
        corners = corners + jitter
    S = 6 if grid == "aff" else 8
    perts = rng.normal(size=(N_SAMPLES, S)) * (SIGMA_A if S == 6 else SIGMA_H) * 2.0
    if S == 8:
        perts[:, 6:] *= 0.25          # (far from the image origin the projective terms alone would throw whole samples out of the frame)
    perts[0] = 0
    return corners, perts


def _oracle_am_kw(am_kw):
    return {{"mi_pou": "pou", "mi_n_bins": "n_bins"}.get(k, k): v for k, v in am_kw.items()}


def reference_rows(oracle, frame, shape, am, grid, corners, perts):
    """-> (oracle's rows, the NumPy walk's rows or None, the oracle's raw pixel values): all float64, all on the CPU"""
    import numpy_ref as R
    resx, resy = shape
    am_id, am_kw = AMS[am]
    ssm = L.SSM_AFFINE if grid == "aff" else L.SSM_HOMOGRAPHY

    def rows(a, **kw):
        o_ssm = oracle.SSM(ssm, resx, resy); o_am = oracle.AM(a, resx, resy, **kw)
        o_am.set_curr_img(frame)
        o_ssm.set_corners(corners)
        o_am.initialize_pix_vals(o_ssm.get("curr_pts"))
        return oracle.nn_generate_dataset(o_am, o_ssm, perts)
    want = rows(am_id, **_oracle_am_kw(am_kw))
    raw = want if am_id == L.AM_SSD else rows(L.AM_SSD)
    walk = None
    if grid != "aff":
        _, init_hm = R.grid_from_corners(corners, resx, resy)
        if am_id == L.AM_MI:
            raw_walk = R.nn_dataset_rows(frame, init_hm, perts, ncc=False)
            walk = np.stack([R.nn_mi_dist_feat(r, am_kw.get("mi_n_bins", 8), bool(am_kw.get("mi_pou", 0))) for r in raw_walk])
        else:
            walk = R.nn_dataset_rows(frame, init_hm, perts, ncc=(am_id == L.AM_NCC))
    return want, walk, raw


def mi_integer_distance(raw, n_bins, pou):
    """the least distance of the reference's normalised pixel values to an integer (the border value 128 maps to x.5 for both configurations)"""
    import numpy_ref as R
    mult, add = R.mi_pix_norm(n_bins, pou)
    v = mult * raw + add
    return float(np.abs(v - np.rint(v)).min())


def _generate_guarded(gpu_ctx, frame, shape, am, grid, corners, perts, mode):
    """the cell's rows through nn_dataset_dev into the middle of a sentinel-filled device buffer -> (rows, guard before, guard after).  An odd
    row length gets an odd guard: its rows then start on 8-byte and not on 16-byte boundaries, as inside any (n, N) matrix."""
    import torch
    am_id, am_kw = AMS[am]
    ssm = L.SSM_AFFINE if grid == "aff" else L.SSM_HOMOGRAPHY
    n = len(perts)
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, am_id, ssm, shape[0], shape[1], 1, **am_kw)
    b.set_math_mode(mode)
    b.set_corners(corners[None]); b.initialize_pix_vals()
    F = b.nn_feature_size()
    g0 = GUARD + (shape[0] * shape[1]) % 2
    buf = torch.full((g0 + n * F + GUARD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    pin = torch.as_tensor(np.ascontiguousarray(perts), device="cuda:0")
    pout = torch.full((n + 2, b.S), SENTINEL, dtype=torch.float64, device="cuda:0")
    d = b.nn_desc(n, SIGMA_H)
    b.nn_dataset_dev(d, buf[g0:].data_ptr(), 0, n, dev_perts_in_ptr=pin.data_ptr(), dev_perts_out_ptr=pout.data_ptr())   # (raises on an error return)
    gpu_ctx.synchronize()
    host = buf.cpu().numpy()
    assert np.array_equal(pout.cpu().numpy()[:n], perts) and np.all(pout.cpu().numpy()[n:] == SENTINEL)
    b.close()
    return host[g0:g0 + n * F].reshape(n, F).copy(), host[:g0], host[g0 + n * F:]


def _compare(got, want, am, N):
    """the project's bounds (test_nn_dataset_rows_follow_oracle): SSD 1e-9 of a pixel value, NCC 1e-12, MI floor row EQUAL and weights 1e-9
    -> max |difference|"""
    am_id = AMS[am][0]
    assert got.shape == want.shape
    if am_id == L.AM_MI:
        assert np.array_equal(got[:, :N], want[:, :N]), "floor row differs at %d entries" % int((got[:, :N] != want[:, :N]).sum())
        np.testing.assert_allclose(got[:, N:], want[:, N:], rtol=0, atol=1e-9)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 if am_id == L.AM_SSD else 1e-12)
    return float(np.abs(got - want).max())


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_nn_rows_across_the_seams(oracle, gpu_ctx, frame, parity_record, cell):
    mode, shape, am, grid, where = cell
    N = shape[0] * shape[1]
    corners, perts = case_inputs(frame, shape, grid, where)
    want, walk, raw = reference_rows(oracle, frame, shape, am, grid, corners, perts)
    if where == "border":
        assert (raw == 128.0).mean() > 0.05            # the samples do leave the frame
    if AMS[am][0] == L.AM_MI:
        assert mi_integer_distance(raw, AMS[am][1].get("mi_n_bins", 8), AMS[am][1].get("mi_pou", 0)) >= MI_INTEGER_MARGIN
    got, before, after = _generate_guarded(gpu_ctx, frame, shape, am, grid, corners, perts, mtf_amd.MATH_FAST if mode == "fast" else mtf_amd.MATH_REPLAY)
    assert np.all(before == SENTINEL), "the kernel wrote in front of the first row"
    assert np.all(after == SENTINEL), "the kernel wrote past the last row (first at +%d)" % int(np.argmax(after != SENTINEL))
    assert not np.any(got == SENTINEL), "entries of the rows were never written"
    e_oracle = _compare(got, want, am, N)
    e_walk = _compare(got, walk, am, N) if walk is not None else None
    parity_record.append(dict(test="nn_rows_across_the_seams", cell=_cell_id(cell), max_abs_vs_oracle=e_oracle, max_abs_vs_numpy_walk=e_walk))


def persistent_inputs(shape):
    """1300 samples of a template inside the frame (the seed's base chosen on the reference, as case_inputs': test_nn_shapes_cpu.py)"""
    rng = np.random.default_rng(4909 + SHAPES.index(shape))
    corners = synth.square_corners(256.0, 256.0, 100) + rng.uniform(-2, 2, size=(2, 4))
    return corners, rng.normal(size=(1300, 8)) * SIGMA_H


@pytest.mark.parametrize("shape,am", [((64, 48), "ncc"), ((81, 79), "ssd"), ((59, 53), "mi10pou")], ids=["64x48-ncc", "81x79-ssd", "59x53-mi10pou"])
def test_nn_rows_persistent_rounds_at_long_rows(oracle, gpu_ctx, frame, shape, am):
    """more samples than the device holds workgroups of 72 KB (two per compute unit): every workgroup walks several samples per chunk -- NCC's
    alternating sum slots at a full chunk, the sample loop restarted per chunk for the longer rows -- against the oracle on the same samples"""
    corners, perts = persistent_inputs(shape)
    n = len(perts)
    am_id, am_kw = AMS[am]
    o_ssm = oracle.SSM(L.SSM_HOMOGRAPHY, *shape); o_am = oracle.AM(am_id, *shape, **_oracle_am_kw(am_kw))
    o_am.set_curr_img(frame); o_ssm.set_corners(corners); o_am.initialize_pix_vals(o_ssm.get("curr_pts"))
    want = oracle.nn_generate_dataset(o_am, o_ssm, perts)
    if am_id == L.AM_MI:
        o_raw = oracle.AM(L.AM_SSD, *shape); o_raw.set_curr_img(frame); o_ssm.set_corners(corners); o_raw.initialize_pix_vals(o_ssm.get("curr_pts"))
        assert mi_integer_distance(oracle.nn_generate_dataset(o_raw, o_ssm, perts), 10, 1) >= MI_INTEGER_MARGIN
    gpu_ctx.set_image(frame)
    ds = NNDataset(gpu_ctx, am=am_id, ssm=L.SSM_HOMOGRAPHY, resx=shape[0], resy=shape[1], n_samples=n, am_params=am_kw)
    got = ds.initialize(corners, perts)
    _compare(got, want, am, shape[0] * shape[1])
    ds.batch.close()


def test_nn_two_launch_switch_for_ncc_rows(oracle, gpu_ctx, frame):
    """NCC rows of 3072 entries take the two-launch form, of 3127 the workgroup form (nn_two_launch_ok): both sides of the switch against one
    reference, and each against the other math mode, which does not switch"""
    for shape in ((64, 48), (59, 53)):
        corners, perts = case_inputs(frame, shape, "homq", "inside")
        want, walk, _ = reference_rows(oracle, frame, shape, "ncc", "homq", corners, perts)
        rows = {}
        for mode in (mtf_amd.MATH_FAST, mtf_amd.MATH_REPLAY):
            rows[mode], before, after = _generate_guarded(gpu_ctx, frame, shape, "ncc", "homq", corners, perts, mode)
            assert np.all(before == SENTINEL) and np.all(after == SENTINEL)
            np.testing.assert_allclose(rows[mode], want, rtol=0, atol=1e-12)
            np.testing.assert_allclose(rows[mode], walk, rtol=0, atol=1e-12)
            np.testing.assert_allclose(np.linalg.norm(rows[mode], axis=1), 1.0, rtol=1e-12)
            np.testing.assert_allclose(rows[mode].sum(axis=1), 0.0, atol=1e-10)
        np.testing.assert_allclose(rows[mtf_amd.MATH_FAST], rows[mtf_amd.MATH_REPLAY], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------------------
# B. the row kernel's dynamic-LDS attribute and the order of the calls

def _rows_unit_z_off(gpu_ctx, frame, am, ssm, shape, corners, perts):
    """rows of a batch whose grid is NOT unit-z: a homography template with general-quadrilateral corners is that by itself; an affine one
    becomes it when the caller supplies its own homogeneous grid (mtfhip_batch_write of INIT_HXY / INIT_Z) -- here the batch's own points
    with z = 1, so that the rows are those of the unit-z grid and the oracle stays the reference"""
    am_id, am_kw = AMS[am]
    gpu_ctx.set_image(frame)
    b = mtf_amd.Batch(gpu_ctx, am_id, ssm, shape[0], shape[1], 1, **am_kw)
    b.set_corners(corners[None]); b.initialize_pix_vals()
    if ssm == L.SSM_AFFINE:
        pts = b.read(L.BUF_INIT_PTS)
        b.write(L.BUF_INIT_HXY, pts); b.write(L.BUF_INIT_Z, np.ones((1, shape[0] * shape[1])))
    p, f = b.nn_dataset(len(perts), SIGMA_H, None, seed=0, perturbations=perts)      # (raises on an error return)
    assert np.array_equal(p, perts)
    b.close()
    return f


@pytest.mark.parametrize("am", ["ssd", "ncc", "mi10pou"])
def test_nn_lds_attribute_does_not_depend_on_call_order(oracle, gpu_ctx, frame, am):
    """a 72 KB launch (non-unit-z, 3072 LDS entries of 24 bytes: more than a launch gets without the kernel's MaxDynamicSharedMemorySize), then
    a small one (N = 576: 1024 entries, 24 KB) on the same kernel instantiation, then the 72 KB shape again -- on one (SSM, AM), then on the
    other SSM: every call returns without an error and every result is the reference's.  (With the attribute set only on a miss of a cache
    keyed by the LDS size, the small call lowers it again; a runtime that enforces the attribute then refuses the third call.  The runtime
    this was first run on accepts all three either way -- the 72 KB launch works, and had never been run -- so here the test pins the
    results and the error returns of the sequence, not the refusal.)"""
    big, small = (64, 48), (24, 24)
    for ssm, grid in ((L.SSM_HOMOGRAPHY, "homq"), (L.SSM_AFFINE, "aff")):
        for step, shape in enumerate((big, small, big)):
            corners, perts = case_inputs(frame, SHAPES[step], grid, "inside")     # (three different sample sets; the shape is the step's)
            want, walk, raw = reference_rows(oracle, frame, shape, am, grid, corners, perts)
            if am == "mi10pou":
                assert mi_integer_distance(raw, 10, 1) >= MI_INTEGER_MARGIN
            got = _rows_unit_z_off(gpu_ctx, frame, am, ssm, shape, corners, perts)
            _compare(got, want, am, shape[0] * shape[1])
            if walk is not None:
                _compare(got, walk, am, shape[0] * shape[1])


# ------------------------------------------------------------------------------------------------------------------------------
# C. NNDataset.initialize_sharded

SHARD_AMS = {"ssd": (L.AM_SSD, {}), "ncc": (L.AM_NCC, {}), "mi10pou": (L.AM_MI, dict(mi_n_bins=10, mi_pou=1))}
SHARD_CORNERS = synth.square_corners(250.0, 262.0, 90) + np.array([[0.7, -1.1, 0.4, 1.3], [-0.6, 0.9, 1.2, -0.8]])
TWO_DISTR = dict(ssm_sigma=(SIGMA_H * 0.1, SIGMA_H), ssm_mean=(np.zeros(8), np.array([0.001, 0, 0.5, 0, -0.001, -0.25, 0, 0])))


def _dataset(ctx, am, n, distr):
    am_id, am_kw = SHARD_AMS[am]
    kw = dict(ssm_sigma=SIGMA_H)
    if distr == 2:
        kw = dict(TWO_DISTR, distr_n_samples=[n * 2 // 5, n - n * 2 // 5])
    return NNDataset(ctx, am=am_id, ssm=L.SSM_HOMOGRAPHY, resx=24, resy=24, n_samples=n, seed=31, am_params=am_kw, **kw)


@pytest.mark.parametrize("distr", [1, 2], ids=["one_distribution", "two_distributions"])
@pytest.mark.parametrize("am", list(SHARD_AMS))
def test_nn_initialize_sharded_world_1_equals_initialize(gpu_ctx, frame, am, distr):
    """one rank: features and perturbations BIT-IDENTICAL to initialize() with the same seed (several distributions: consecutive row blocks
    seeded seed + k, as initialize lays them out), `features` in the form nearest() takes, the device matrix returned"""
    n = 1001
    gpu_ctx.set_image(frame)
    ref = _dataset(gpu_ctx, am, n, distr)
    f = ref.initialize(SHARD_CORNERS)
    ds = _dataset(gpu_ctx, am, n, distr)
    dev = ds.initialize_sharded(SHARD_CORNERS)
    assert dev.is_cuda and tuple(dev.shape) == f.shape == (n, ds.feature_size())
    assert isinstance(ds.features, np.ndarray) and np.array_equal(ds.features, f) and np.array_equal(dev.cpu().numpy(), f)
    assert ds.perturbations.shape == (n, 8) and np.array_equal(ds.perturbations, ref.perturbations)
    assert ds.nearest(f[777]) == (777, 0.0)
    ref.batch.close(); ds.batch.close()


@pytest.mark.parametrize("world,n", [(2, 1001), (3, 1001), (8, 1001), (8, 5)])
@pytest.mark.parametrize("am,distr", [("ssd", 1), ("ssd", 2), ("ncc", 1), ("mi10pou", 2)])
def test_nn_initialize_sharded_loopback_equals_initialize(gpu_ctx, frame, world, n, am, distr):
    """`world` ranks as threads of this process over a loopback communicator (the pattern of test_pf_sharded_loopback_equals_unsharded): ragged
    and -- world > n -- EMPTY shards (count 0 is a no-op), one in-place all-gather of the padded row blocks and one of the perturbations;
    every rank ends with matrix and perturbations bit-identical to the unsharded initialize(), the pad rows never reach them"""
    from mtf_amd.sm import Comm
    from test_gpu_trackers import _run_ranks
    gpu_ctx.set_image(frame)
    ref = _dataset(gpu_ctx, am, n, distr)
    f = ref.initialize(SHARD_CORNERS)
    p = ref.perturbations
    ref.batch.close()

    def run(comm):
        ctx = mtf_amd.Context(0)
        ctx.set_image(frame)
        ds = _dataset(ctx, am, n, distr)
        dev = ds.initialize_sharded(SHARD_CORNERS, comm=comm)
        out = (ds.features.copy(), ds.perturbations.copy(), tuple(dev.shape))
        ds.batch.close(); ctx.close()
        return out
    comms = Comm.loopback(world)
    got = _run_ranks(world, lambda r: run(comms[r]))
    for c in comms:
        c.close()
    for r in range(world):
        assert got[r][2] == f.shape == got[r][0].shape, "rank %d: shape" % r
        assert np.array_equal(got[r][0], f), "rank %d: features differ from the unsharded matrix" % r
        assert np.array_equal(got[r][1], p), "rank %d: perturbations differ from the unsharded ones" % r


# ------------------------------------------------------------------------------------------------------------------------------
# D. NNDataset.nearest

def _brute_force(features, q):
    """(index of the nearest row, its squared distance, the second smallest squared distance) in extended precision"""
    d = ((features.astype(np.longdouble) - q.astype(np.longdouble)[None]) ** 2).sum(axis=1)
    order = np.argsort(d, kind="stable")
    return int(order[0]), d[order[0]], d[order[1]]


@pytest.mark.parametrize("how", ["initialize", "initialize_sharded"])
@pytest.mark.parametrize("am", ["ssd", "ncc"])
def test_nn_nearest_equals_brute_force(gpu_ctx, frame, am, how):
    """queries that are NOT stored rows (rows of a second dataset drawn with another seed) against an exhaustive search in np.longdouble: the
    same index wherever the reference's best and second-best distances differ by more than a relative 1e-12 (checked on the reference for
    every query), the distance to rtol 1e-12; and a deliberate tie -- a duplicated row -- goes to the first index"""
    n, nq = 600, 40
    am_id, _ = SHARD_AMS[am]
    gpu_ctx.set_image(frame)
    ds = NNDataset(gpu_ctx, am=am_id, resx=24, resy=24, n_samples=n, ssm_sigma=SIGMA_H, seed=5)
    if how == "initialize":
        ds.initialize(SHARD_CORNERS)
    else:
        ds.initialize_sharded(SHARD_CORNERS)
    qs = NNDataset(gpu_ctx, am=am_id, resx=24, resy=24, n_samples=nq, ssm_sigma=SIGMA_H, seed=6)
    queries = qs.initialize(SHARD_CORNERS)
    assert not np.array_equal(qs.perturbations[:, :], ds.perturbations[:nq])
    for q in queries:
        k_ref, d_ref, d_second = _brute_force(ds.features, q)
        assert d_ref > 0 and d_second - d_ref > 1e-12 * d_second          # not a stored row; the reference's choice is unambiguous
        k, d = ds.nearest(q)
        assert k == k_ref
        assert abs(np.longdouble(d) - d_ref) <= 1e-12 * d_ref
    # the tie: row 57 again at 311 and at 599; a query near it (not equal to it) is equally far from all three
    ds.features = ds.features.copy()
    ds.features[311] = ds.features[57]; ds.features[599] = ds.features[57]
    q = ds.features[57] + 1e-3 * (queries[0] - ds.features[57])
    k_ref, d_ref, d_second = _brute_force(ds.features, q)
    assert k_ref == 57 and d_second == d_ref
    k, d = ds.nearest(q)
    assert k == 57 and abs(np.longdouble(d) - d_ref) <= 1e-12 * d_ref
    ds.batch.close(); qs.batch.close()
