"""SCV (the Sum of Conditional Variance appearance model) on CPU: the fixture tests/golden/lk_golden6.npz and its float64 definitions
(tests/golden/make_golden6.py) held to themselves, and the C ABI the device path adds for it.

- the two-sums-per-template-bin map (what k_scv_hist of kernels_imap.hip computes) equals the literal n_bins^2 joint-histogram map: bit for bit with
  Dirac histograms, within 1e-13 relative with Bilinear ones, and both equal the fixture's map;
- with the map frozen, g = df/dIt . Jt is the derivative of f over the state (a central difference through the compositional update);
- the new symbols and MTFHIP_AM_SCV are exported and mtfhip_patch_desc keeps its layout."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden6", os.path.join(GOLDEN, "make_golden6.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = _gen()
R = M.R
G = np.load(os.path.join(GOLDEN, "lk_golden6.npz"))
TAGS = [str(t) for t in G["tags"]]


def case(tag):
    ht, nb, lin, resx, resy, aff = (int(v) for v in G[tag + "_cfg"])
    pa = M.Patch(G["img"].astype(np.float64), nb, resx, resy, bool(aff), G[tag + "_corners"])
    return ht, nb, lin, pa


@pytest.mark.parametrize("tag", TAGS)
def test_per_bin_map_equals_joint_histogram_map(tag):
    ht, nb, lin, pa = case(tag)
    It, _ = pa.sample(pa.warp(G[tag + "_p"]))
    lit = M.literal_map(It, pa.I0o, nb, ht)
    pb = M.per_bin_map(It, pa.I0o, nb, ht)
    np.testing.assert_array_equal(lit, G[tag + "_map"])
    np.testing.assert_array_equal(pa.I0o[:16], G[tag + "_I0o_head"])
    if ht == 0:
        np.testing.assert_array_equal(pb, lit)
    else:
        np.testing.assert_allclose(pb, lit, rtol=1e-13, atol=0)
    # the fixture exercises the empty-bin rule: bins no template pixel falls in map to themselves
    empty = np.bincount(pa.I0o.astype(np.int64), minlength=nb)[:nb] == 0
    if ht == 0:
        assert empty.any(), tag
        np.testing.assert_array_equal(lit[empty], np.arange(nb)[empty])


@pytest.mark.parametrize("tag", ["d64n_50", "b64l_50", "d7n_37x23", "d64n_aff"])
def test_gradient_is_derivative_with_frozen_map(tag):
    """f(p) = -|It(W(p)) - I0|^2 / 2 with I0 = map(I0_orig) held fixed: g = df/dIt . Jt against a central difference along each
    parameter of the compositional update W(p) . dW(d), d = +-h e_s"""
    ht, nb, lin, pa = case(tag)
    W = pa.warp(G[tag + "_p"])
    It, Jt = pa.sample(W)
    I0 = M.remap(pa.I0o, M.literal_map(It, pa.I0o, nb, ht), lin)
    np.testing.assert_array_equal(I0[:16], G[tag + "_I0_head"])
    g = -(It - I0) @ Jt
    np.testing.assert_allclose(g, G[tag + "_g"], rtol=1e-12, atol=0)

    def f_at(d):
        Wd = W @ (R.aff_matrix(d) if pa.affine else R.hom_matrix(d))
        Itd, _ = pa.sample(Wd)
        r = Itd - I0
        return -0.5 * float(r @ r)

    S = Jt.shape[1]
    scale = np.abs(g).max()
    for s in range(S):
        h = 1e-4 / max(np.abs(Jt[:, s]).max(), 1e-300)
        e = np.zeros(S)
        e[s] = h
        fd = (f_at(e) - f_at(-e)) / (2 * h)
        assert abs(fd - g[s]) <= 2e-3 * max(abs(g[s]), 1e-3 * scale), (s, fd, g[s])


def test_scv_abi_symbols_exported():
    from mtf_amd import _lib as L
    assert L.AM_SCV == 3
    assert (L.SCV_HIST_DIRAC, L.SCV_HIST_BILINEAR, L.SCV_HIST_BSPLINE) == (0, 1, 2)
    for s in ("mtfhip_batch_set_scv", "mtfhip_batch_scv_intensity_map"):
        assert s in L.SYMBOLS
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in L.SYMBOLS:
        assert hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    assert "MTFHIP_AM_SCV = 3" in hdr
    assert "MTFHIP_BUF_COUNT = 22" in hdr
    import mtf_amd
    assert mtf_amd.AM_SCV == 3 and hasattr(mtf_amd.Batch, "set_scv") and hasattr(mtf_amd.Batch, "scv_intensity_map")


# mtfhip_patch_desc as it was before SCV (x86-64 / SysV): the struct is unchanged
DESC_LAYOUT = dict(size=72, am=0, ssm=4, resx=8, resy=12, grad_eps=16, likelihood_alpha=24, mi_n_bins=32, mi_pre_seed=40,
                   mi_partition_of_unity=48, hess_eps=56, n_channels=64)


def test_patch_desc_layout_unchanged():
    from mtf_amd import _lib as L
    assert ctypes.sizeof(L.PatchDesc) == DESC_LAYOUT["size"]
    for name, off in DESC_LAYOUT.items():
        if name != "size":
            assert getattr(L.PatchDesc, name).offset == off, name


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_patch_desc_layout_from_header(tmp_path):
    """the header itself, compiled: sizeof / offsetof of every field"""
    src = tmp_path / "desc.c"
    fields = [k for k in DESC_LAYOUT if k != "size"]
    body = "".join('printf("%%s %%zu\\n", "%s", offsetof(mtfhip_patch_desc, %s));' % (f, f) for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtfhip.h"\nint main(void){printf("size %%zu\\n", sizeof(mtfhip_patch_desc));%s'
                   'return MTFHIP_AM_SCV == 3 ? 0 : 1;}\n' % body)
    exe = tmp_path / "desc"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}
    assert got == DESC_LAYOUT
