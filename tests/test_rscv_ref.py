"""RSCV (the Reversed Sum of Conditional Variance appearance model) on CPU: the fixture tests/golden/lk_golden7.npz and its float64
definitions (tests/golden/make_golden7.py) held to themselves, and the C ABI the device path adds for it.

- the two-integer-sums-per-current-bin map (what k_rscv_hist of kernels_imap.hip computes) equals the literal n_bins^2 joint-histogram map bit for bit,
  and both equal the fixture's map;
- with the map frozen, g = df/dIt . Jt is the derivative of f over the state (a central difference through the compositional update);
- the new symbols and MTFHIP_AM_RSCV are exported and mtfhip_patch_desc keeps its layout."""
import ctypes
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _gen():
    sys.path.insert(0, GOLDEN)   # (make_golden7 imports make_golden5 / make_golden6 next to it)
    spec = importlib.util.spec_from_file_location("make_golden7", os.path.join(GOLDEN, "make_golden7.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = _gen()
R = M.R
G = np.load(os.path.join(GOLDEN, "lk_golden7.npz"))
TAGS = [str(t) for t in G["tags"]]


def case(tag):
    nb, lin, resx, resy, aff = (int(v) for v in G[tag + "_cfg"])
    pa = M.Patch(G["img"].astype(np.float64), nb, resx, resy, bool(aff), G[tag + "_corners"])
    return nb, lin, pa


def test_fixture_image_has_no_whole_flat_levels():
    """the issue the fixture avoids: a flat region at a level that normalises to a whole number puts (int)It_orig on rounding"""
    img = G["img"].astype(np.float64)
    assert not np.any(img == 255.0)
    for nb in (7, 64, 256):
        v = img[img > 0] * ((nb - 1.0) / 255.0)
        assert not np.any(v == np.round(v)), nb


@pytest.mark.parametrize("tag", TAGS)
def test_per_bin_map_equals_joint_histogram_map(tag):
    nb, lin, pa = case(tag)
    It_orig, _ = pa.sample(pa.warp(G[tag + "_p"]))
    np.testing.assert_array_equal(It_orig[:16], G[tag + "_It_orig_head"])
    lit = M.literal_map(It_orig, pa.I0o, nb)
    pb = M.per_bin_map(It_orig, pa.I0o, nb)
    np.testing.assert_array_equal(lit, G[tag + "_map"])
    np.testing.assert_array_equal(pb, lit)
    It = M.remap(It_orig, lit, lin)
    np.testing.assert_array_equal(It[:16], G[tag + "_It_head"])
    if tag + "_It" in G:
        np.testing.assert_array_equal(It, G[tag + "_It"])
    # bins no current pixel falls in map to themselves
    empty = np.bincount(It_orig.astype(np.int64), minlength=nb)[:nb] == 0
    np.testing.assert_array_equal(lit[empty], np.arange(nb)[empty])
    # a populated bin maps to a mean of template bins: inside [0, n_bins - 1]
    assert lit.min() >= 0 and lit.max() <= nb - 1


def test_fixture_exercises_the_empty_bin_rule():
    hit = 0
    for tag in TAGS:
        nb, _, pa = case(tag)
        It_orig, _ = pa.sample(pa.warp(G[tag + "_p"]))
        hit += int(np.any(np.bincount(It_orig.astype(np.int64), minlength=nb)[:nb] == 0))
    assert hit >= 3


@pytest.mark.parametrize("tag", ["r64n_50", "r64l_50", "r7n_37x23", "r64n_aff"])
def test_gradient_is_derivative_with_frozen_map(tag):
    """g = df/dIt . Jt with Jt the unmapped image's (mapped_gradient 0) is the derivative of f with the map frozen as the offset it
    applies at the current state, f(p) = -|It_orig(W(p)) + (It - It_orig) - I0|^2 / 2: against a central difference along each parameter
    of the compositional update W(p) . dW(d), d = +-h e_s"""
    nb, lin, pa = case(tag)
    W = pa.warp(G[tag + "_p"])
    It_orig, Jt = pa.sample(W)
    It = M.remap(It_orig, M.literal_map(It_orig, pa.I0o, nb), lin)
    g = -(It - pa.I0o) @ Jt
    np.testing.assert_allclose(g, G[tag + "_g"], rtol=1e-12, atol=0)
    off = It - It_orig

    def f_at(d):
        Wd = W @ (R.aff_matrix(d) if pa.affine else R.hom_matrix(d))
        Itd, _ = pa.sample(Wd)
        r = Itd + off - pa.I0o
        return -0.5 * float(r @ r)

    assert f_at(np.zeros(Jt.shape[1])) == pytest.approx(float(G[tag + "_f"]), rel=1e-12)
    S = Jt.shape[1]
    scale = np.abs(g).max()
    for s in range(S):
        h = 1e-5 / max(np.abs(Jt[:, s]).max(), 1e-300)   # (short: fewer samples cross a bilinear cell edge inside the difference)
        e = np.zeros(S)
        e[s] = h
        fd = (f_at(e) - f_at(-e)) / (2 * h)
        assert abs(fd - g[s]) <= 2e-3 * max(abs(g[s]), 1e-3 * scale), (s, fd, g[s])


def test_rscv_abi_symbols_exported():
    from mtf_amd import _lib as L
    assert L.AM_RSCV == 4
    for s in ("mtfhip_batch_set_rscv", "mtfhip_batch_rscv_intensity_map"):
        assert s in L.SYMBOLS
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in L.SYMBOLS:
        assert hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "mtfhip.h")).read()
    assert "MTFHIP_AM_RSCV = 4" in hdr
    assert "MTFHIP_BUF_COUNT = 22" in hdr
    import mtf_amd
    assert mtf_amd.AM_RSCV == 4 and hasattr(mtf_amd.Batch, "set_rscv") and hasattr(mtf_amd.Batch, "rscv_intensity_map")
    from mtf_amd import host
    assert hasattr(host.CppTracker, "rscv")


# mtfhip_patch_desc as it was before RSCV (x86-64 / SysV): the struct is unchanged
DESC_LAYOUT = dict(size=72, am=0, ssm=4, resx=8, resy=12, grad_eps=16, likelihood_alpha=24, mi_n_bins=32, mi_pre_seed=40,
                   mi_partition_of_unity=48, hess_eps=56, n_channels=64)


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_patch_desc_layout_from_header_rscv(tmp_path):
    """the header itself, compiled: sizeof / offsetof of every field, and the new enumerator"""
    src = tmp_path / "desc.c"
    fields = [k for k in DESC_LAYOUT if k != "size"]
    body = "".join('printf("%%s %%zu\\n", "%s", offsetof(mtfhip_patch_desc, %s));' % (f, f) for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtfhip.h"\nint main(void){printf("size %%zu\\n", sizeof(mtfhip_patch_desc));%s'
                   'int (*s)(mtfhip_batch *, int, int, int) = mtfhip_batch_set_rscv; int (*m)(mtfhip_batch *, double *) = mtfhip_batch_rscv_intensity_map;'
                   '(void)s; (void)m; return MTFHIP_AM_RSCV == 4 ? 0 : 1;}\n' % body)
    obj = tmp_path / "desc.o"
    subprocess.check_call(["cc", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(obj), str(src)])
    # (compiled only against the declarations: the layout is printed by a second program that needs no library)
    src2 = tmp_path / "desc2.c"
    src2.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtfhip.h"\nint main(void){printf("size %%zu\\n", sizeof(mtfhip_patch_desc));%s'
                    'return MTFHIP_AM_RSCV == 4 ? 0 : 1;}\n' % body)
    exe = tmp_path / "desc2"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src2)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = {out[i]: int(out[i + 1]) for i in range(0, len(out), 2)}
    assert got == DESC_LAYOUT
