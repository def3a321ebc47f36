"""The CPU side of tests/test_gpu_nn_shapes.py: what can be settled without a device.
 - the inputs of every cell keep the REFERENCE's normalised pixel values at least MI_INTEGER_MARGIN from an integer (the condition under
   which the MI floor row must be equal, not a measurement of the kernel), the border cells do cross the border, and the two float64
   references (the oracle's generateDataset, the NumPy walk) agree with each other far inside the bounds the kernel is held to;
 - NNDataset.initialize_sharded refuses a device that is not a GPU before it touches the native layer."""
import numpy as np
import pytest

from mtf_amd import _lib as L
from mtf_amd.sm import NNDataset
import test_gpu_nn_shapes as T


def _geometries():
    seen, out = set(), []
    for _, shape, _, grid, where in T.CELLS:
        if (shape, grid, where) not in seen:
            seen.add((shape, grid, where)); out.append((shape, grid, where))
    return out


def test_cells_cover_every_shape_and_am_in_both_math_modes():
    for mode in ("fast", "replay"):
        assert {(c[1], c[2]) for c in T.CELLS if c[0] == mode} == {(s, a) for s in T.SHAPES for a in T.AMS}
    assert {(c[3], c[4]) for c in T.CELLS} == {(g, w) for g in ("homq", "homsq", "aff") for w in ("inside", "border")}


@pytest.mark.parametrize("shape,grid,where", _geometries(), ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_reference_values_of_every_cell(oracle, frame, shape, grid, where):
    corners, perts = T.case_inputs(frame, shape, grid, where)
    want, walk, raw = T.reference_rows(oracle, frame, shape, "ssd", grid, corners, perts)
    assert raw is want
    border = float((raw == 128.0).mean())
    assert border > 0.05 if where == "border" else border == 0.0
    assert (raw == 128.0).mean(axis=1).max() < 0.98       # no sample is outside the frame altogether (its NCC row would be 0 / 0)
    for n_bins, pou in ((8, 0), (10, 1)):
        assert T.mi_integer_distance(raw, n_bins, pou) >= T.MI_INTEGER_MARGIN
    if walk is not None:
        # two float64 evaluations of the same rows (different operation orders): 1e-11 of a pixel value observed, the kernel's bound is 1e-9
        np.testing.assert_allclose(walk, want, rtol=0, atol=1e-10)
        ncc_o, ncc_w, _ = T.reference_rows(oracle, frame, shape, "ncc", grid, corners, perts)
        assert np.isfinite(ncc_o).all() and np.isfinite(ncc_w).all()
        np.testing.assert_allclose(ncc_w, ncc_o, rtol=0, atol=1e-13)      # (the kernel's bound: 1e-12)


def test_reference_values_of_the_long_mi_case(oracle, frame):
    """the 1300-sample MI case of test_nn_rows_persistent_rounds_at_long_rows, and the three steps of the LDS-attribute test"""
    corners, perts = T.persistent_inputs((59, 53))
    _, _, raw = T.reference_rows(oracle, frame, (59, 53), "ssd", "homq", corners, perts)
    assert T.mi_integer_distance(raw, 10, 1) >= T.MI_INTEGER_MARGIN
    for grid in ("homq", "aff"):
        for step, shape in enumerate(((64, 48), (24, 24), (64, 48))):
            corners, perts = T.case_inputs(frame, T.SHAPES[step], grid, "inside")
            _, _, raw = T.reference_rows(oracle, frame, shape, "ssd", grid, corners, perts)
            assert T.mi_integer_distance(raw, 10, 1) >= T.MI_INTEGER_MARGIN


class _NoNative:
    """stands where the batch is: any use of it is a use of the native layer"""
    def __init__(self, ctx=None):
        self.__dict__["ctx"] = ctx

    def __getattr__(self, name):
        raise AssertionError("initialize_sharded touched the native layer (%s) before refusing the device" % name)


class _Ctx:
    pass


@pytest.mark.parametrize("device", ["cpu", "meta", None])
def test_initialize_sharded_refuses_a_device_that_is_no_gpu(device):
    import torch
    ds = NNDataset.__new__(NNDataset)
    ds.batch = _NoNative(ctx=_Ctx())       # (a context that names no device: None cannot be resolved)
    ds.n, ds.S, ds.seed, ds.sigmas, ds.means, ds.distr_n_samples = 5, 8, 0, [np.ones(8)], [np.zeros(8)], [5]
    ds.features = ds.perturbations = None
    corners = np.array([[10.0, 60.0, 60.0, 10.0], [10.0, 10.0, 60.0, 60.0]])
    with pytest.raises(ValueError, match="GPU device|no device"):
        ds.initialize_sharded(corners, device=device if device is None else torch.device(device))
    assert ds.features is None and ds.perturbations is None
    # a GPU device passes this check (and nothing else is looked at by it)
    assert NNDataset._shard_device("cuda:0", None).type == "cuda"
    ctx = _Ctx(); ctx.device = 0
    assert NNDataset._shard_device(None, _NoNative(ctx=ctx)) == torch.device("cuda", 0)
