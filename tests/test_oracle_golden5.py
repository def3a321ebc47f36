"""CPU: the C++ oracle's MI at 10 bins with partition of unity -- the shipped configuration -- and at 10 / 9 / 5 bins against the
independent NumPy definitions (tests/golden/lk_golden5.npz, generator tests/golden/make_golden5.py): saturated regions (values exactly
on a class boundary, the truncated window at bin 0), a ramp of two or three classes, texture, ragged 37 x 23 patches, an affine case.

Tolerances are test_oracle_golden.py's MI ones: f 1e-10 relative, df/dIt rtol 1e-8, g and H 1e-5 relative (the reference's 1e-8
finite-difference gradient is in Jt and J0)."""
import os

import numpy as np
import pytest

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lk_golden5.npz"))
TAGS = [str(t) for t in G["tags"]]


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def cfg(tag):
    nb, pou, resx, resy, aff = (int(v) for v in G[tag + "_cfg"])
    return nb, pou, resx, resy, bool(aff)


def test_fixture_covers_the_kernel_edges():
    """the cases hold what they are there for: the shipped configuration, values exactly on a class boundary (1.0 with pou, 0.0
    without), and 9 / 5 bins"""
    seen = {cfg(t)[:2] for t in TAGS}
    assert {(10, 1), (10, 0), (9, 1), (5, 0)} <= seen
    assert np.any(G["b10p_sat_I0n_head"] == 1.0) and np.any(G["b10p_sat_Itn_head"] == 1.0)
    assert np.any(G["b10n_sat_I0n_head"] == 0.0) and np.any(G["b10n_sat_Itn_head"] == 0.0)
    assert G["img"].dtype == np.float32 and G["img"].shape == (256, 256)


@pytest.mark.parametrize("tag", TAGS)
def test_mi_golden5(oracle, tag):
    nb, pou, resx, resy, aff = cfg(tag)
    ssm = oracle.SSM(oracle.SSM_AFF if aff else oracle.SSM_HOM, resx, resy)
    am = oracle.AM(oracle.AM_MI, resx, resy, n_bins=nb, pou=pou)
    am.set_curr_img(G["img"])
    ssm.set_corners(G[tag + "_corners"])
    pts0 = ssm.get("curr_pts")
    am.initialize_pix_vals(pts0); am.initialize_pix_grad_pts(pts0)
    am.initialize_similarity(); am.initialize_grad(); am.initialize_hess()
    np.testing.assert_allclose(am.get("I0")[:16], G[tag + "_I0n_head"], rtol=0, atol=1e-10)
    J0 = ssm.cmpt_warped_pix_jacobian(am.get("dI0_dx"))
    # the constant Hessian of init_template: cmptSelfHessian(J0) at the template state, where it is cmptInitHessian(J0)
    assert rel(am.cmpt_self_hessian(J0), G[tag + "_H_init0"]) < 1e-5
    ssm.set_state(G[tag + "_p"])
    pts = ssm.get("curr_pts")
    am.update_pix_vals(pts); am.update_pix_grad_pts(pts)
    am.update_similarity(False); am.update_curr_grad(); am.update_init_grad()
    np.testing.assert_allclose(am.get("It")[:16], G[tag + "_Itn_head"], rtol=0, atol=1e-10)
    assert abs(am.similarity - float(G[tag + "_f"])) <= 1e-10 * abs(float(G[tag + "_f"]))
    np.testing.assert_allclose(am.get("df_dIt")[:16], G[tag + "_df_dIt_head"], rtol=1e-8, atol=1e-14)
    Jt = ssm.cmpt_warped_pix_jacobian(am.get("dIt_dx"))
    assert rel(am.cmpt_curr_jacobian(Jt), G[tag + "_g_curr"]) < 1e-5
    assert rel(am.cmpt_curr_hessian(Jt), G[tag + "_H_curr"]) < 1e-5
    assert rel(am.cmpt_init_hessian(J0), G[tag + "_H_init"]) < 1e-5
    assert rel(am.cmpt_self_hessian(Jt), G[tag + "_H_self1"]) < 1e-5


def test_golden5_generator_is_reproducible(tmp_path):
    """The committed fixture is exactly what the committed generator produces."""
    import shutil
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gen = os.path.join(root, "tests", "golden", "make_golden5.py")
    keep = os.path.join(root, "tests", "golden", "lk_golden5.npz")
    backup = tmp_path / "orig.npz"
    shutil.copy(keep, backup)
    try:
        subprocess.check_call([sys.executable, gen], stdout=subprocess.DEVNULL)
        new = np.load(keep)
        old = np.load(backup)
        assert sorted(new.files) == sorted(old.files)
        for k in new.files:
            assert np.array_equal(new[k], old[k]), k
    finally:
        shutil.copy(backup, keep)
